"""The callers either side of the hot path (SURVEY.md §8f "next" rows), on the device.

* input pipeline — ``transforms.Resize((224,224)) → ToTensor → Normalize(ImageNet)`` of
  `/root/reference/src/testing.py:99-104` (and the 160×160 / 0.5-0.5 variant of `src/app.py:39-42`):
  the resize runs on the device (``resize.resize_bilinear_u8``, bit-exact with Pillow's bilinear resampler, which is what
  torchvision's PIL backend calls; without a device argument Pillow does it on the host), the uint8 → normalised-float step is
  ``ops.normalize_u8`` or the stem itself (3 bytes per pixel cross PCIe instead of 12);
* single-image prediction — `src/testing.py:532-595` ``predict_image``: Resize → ToTensor → Normalize → forward → softmax → max;
* evaluation step — `src/testing.py:255-283`: forward → softmax → arg-max, with the ArcFace branch
  scoring embeddings against the class centres (`:264-269`; `hyperparameter_tuning.py:1038-1046`);
* Siamese verification — `src/testing.py:170-177`: ``dist = pairwise_distance(out1, out2)``,
  ``pred = dist < 0.5``;
* the accumulate step of that loop and the metric block of `src/advanced_metrics.py` from exact integers kept on the device —
  `ClassificationTally`, `evaluate_stream`, `metrics_from_tally` (one launch per batch, no copy, one synchronisation at the end);
* the one-vs-rest ROC AUC and average precision of that metric block (`testing.py:296-312`, `advanced_metrics.py:85-100`) from
  exact pair counts over a score store kept on the device - `OvrScores`, `ovr_rank_rule`, `ovr_metrics`, `evaluate_stream(auc=True)`.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)     # testing.py:102-103
FACENET_MEAN, FACENET_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)                   # app.py:41


def resize_to_u8(images: Sequence, size: Tuple[int, int] = (224, 224), device=None) -> torch.Tensor:
    """``transforms.Resize(size)`` for PIL input (bilinear): PIL images / HWC uint8 arrays → one uint8 [B, H, W, 3] tensor.
    With ``device`` the decoded images are uploaded at their native size and resized on the GPU
    (`resize.resize_bilinear_u8`, bit-exact with Pillow); without it Pillow does it on the host."""
    from PIL import Image
    if device is not None:
        from . import resize as _resize
        return _resize.resize_bilinear_u8([np.asarray(im.convert("RGB") if isinstance(im, Image.Image) else im, np.uint8)
                                           for im in images], size, device)
    out = np.empty((len(images), size[0], size[1], 3), np.uint8)
    for i, im in enumerate(images):
        if not isinstance(im, Image.Image):
            im = Image.fromarray(np.asarray(im, np.uint8))
        out[i] = np.asarray(im.convert("RGB").resize((size[1], size[0]), Image.BILINEAR))
    return torch.from_numpy(out)


def preprocess(images_u8: torch.Tensor, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda") -> torch.Tensor:
    """uint8 [B, H, W, 3] → fp32 NCHW on the device == ``Normalize(mean, std)(ToTensor()(img))``."""
    return ops.normalize_u8(images_u8.to(device, non_blocking=True), mean, std)[0]


def predict_batch(model, images: torch.Tensor, model_type: str):
    """One evaluation-loop step (`testing.py:255-283`): returns ``(outputs, probs, predicted)`` on the
    device.  ``arcface``: logits = cosine(embedding, class centres) (`testing.py:264-269`)."""
    if model_type == 'arcface':
        emb = model(images)
        outputs, _ = ops.cosine_logits(emb, model.arcface.weight.detach(), s=1.0, want_argmax=False)
    else:
        outputs = model(images)
    probs, pred = ops.softmax_argmax(outputs)
    return outputs, probs, pred


def arcface_validate(model, images: torch.Tensor):
    """`hyperparameter_tuning.py:1038-1046`: logits = s · cos(embedding, class centres); arg-max."""
    emb = model.get_embedding(images)
    return ops.cosine_logits(emb, model.arcface.weight.detach(), s=float(model.arcface.s))


def siamese_verify(model, img1: torch.Tensor, img2: torch.Tensor, thresh: float = 0.5):
    """`testing.py:175-177`: returns ``(dist, pred)`` with ``pred = (dist < thresh)`` as float."""
    out1, out2 = model(img1, img2)
    dist, same = ops.pairwise_distance(out1, out2, thresh)
    return dist, same.to(torch.float32)


# ------------------------------------------------------------------------------------------------
# §8(f)-2: the batched evaluation harness around the path (`src/testing.py:26-394`)
# ------------------------------------------------------------------------------------------------
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')


def image_folder(root: str):
    """``datasets.ImageFolder(root)``'s sample list (`testing.py:110`): classes = sorted sub-directories, samples =
    every image file under each class directory in sorted walk order.  Returns ``(samples, classes)`` with
    ``samples = [(path, class_index), ...]``."""
    import os
    classes = sorted(d.name for d in os.scandir(root) if d.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {root}.")
    samples = []
    for ci, c in enumerate(classes):
        for r, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
            for f in sorted(files):
                if f.lower().endswith(IMG_EXTENSIONS):
                    samples.append((os.path.join(r, f), ci))
    return samples, classes


def _folder_batches(samples, batch_size, device):
    from PIL import Image
    for lo in range(0, len(samples), batch_size):
        chunk = samples[lo: lo + batch_size]
        imgs = []
        for path, _ in chunk:
            with Image.open(path) as im:
                imgs.append(im.convert("RGB"))
        u8 = resize_to_u8(imgs, (224, 224), device=device)                    # transforms.Resize((224, 224)), `testing.py:100`: on the device
        yield preprocess(u8, IMAGENET_MEAN, IMAGENET_STD, device), torch.tensor([c for _, c in chunk], dtype=torch.int64)


def _results_file_name(model_type: str) -> str:
    """`testing.py:369-378`."""
    return {'siamese': 'siamese_network_results.json', 'arcface': 'arcface_model_results.json',
            'baseline': 'baseline_model_results.json', 'cnn': 'cnn_model_results.json'}.get(model_type, f'{model_type}_model_results.json')


def classification_metrics(all_targets: np.ndarray, all_predictions: np.ndarray, all_probs: np.ndarray, siamese: bool = False) -> dict:
    """The metric block of `testing.py:290-315` (sklearn, weighted averages, one-vs-rest ROC AUC, average precision;
    Siamese: curves on ``-distance``).  A metric sklearn cannot define on the given labels (a class with no sample)
    comes back as NaN instead of aborting the evaluation."""
    from sklearn.metrics import (accuracy_score, auc, average_precision_score, f1_score, precision_recall_curve,
                                 precision_score, recall_score, roc_auc_score, roc_curve)

    def safe(fn):
        try:
            return float(fn())
        except Exception:
            return float("nan")

    m = {"accuracy": safe(lambda: accuracy_score(all_targets, all_predictions)),
         "precision": safe(lambda: precision_score(all_targets, all_predictions, average='weighted', zero_division=0)),
         "recall": safe(lambda: recall_score(all_targets, all_predictions, average='weighted', zero_division=0)),
         "f1": safe(lambda: f1_score(all_targets, all_predictions, average='weighted', zero_division=0))}
    if siamese:
        def roc():
            fpr, tpr, _ = roc_curve(all_targets, -all_probs.ravel())
            return auc(fpr, tpr)

        def pr():
            p, r, _ = precision_recall_curve(all_targets, -all_probs.ravel())
            return auc(r, p)
        m["roc_auc"], m["pr_auc"] = safe(roc), safe(pr)
    else:
        m["roc_auc"] = safe(lambda: roc_auc_score(all_targets, all_probs, multi_class='ovr'))
        m["pr_auc"] = safe(lambda: average_precision_score(all_targets, all_probs))
    return m


FAR_TARGETS = (1e-1, 1e-2, 1e-3, 1e-4)


def pair_totals(labels, other_labels=None) -> Tuple[int, int]:
    """(genuine, impostor) pair counts from the label histograms, exact: self mode (``other_labels=None``) counts every unordered
    pair of ``labels`` once, cross mode every (i, j) of ``labels`` x ``other_labels``."""
    la = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels, dtype=np.int64).reshape(-1)
    if other_labels is None:
        _, n = np.unique(la, return_counts=True)
        genuine = sum(int(c) * (int(c) - 1) // 2 for c in n)
        return genuine, len(la) * (len(la) - 1) // 2 - genuine
    lb = np.asarray(other_labels.cpu() if isinstance(other_labels, torch.Tensor) else other_labels, dtype=np.int64).reshape(-1)
    ua, na = np.unique(la, return_counts=True)
    nb = dict(zip(*(x.tolist() for x in np.unique(lb, return_counts=True))))
    genuine = sum(int(c) * nb.get(int(u), 0) for u, c in zip(ua.tolist(), na.tolist()))
    return genuine, len(la) * len(lb) - genuine


def metrics_from_counts(thresholds, accepted, genuine_pairs: int, impostor_pairs: int, far_targets=FAR_TARGETS) -> dict:
    """The verification metrics of exact counts (`ops.verify_counts`): ``accepted`` [2, T] = genuine / impostor pairs accepted at
    each threshold.  tar[k] = G_k / genuine_pairs, far[k] = I_k / impostor_pairs; ``roc_auc`` = trapezoid over (0, 0),
    (far_k, tar_k)..., (1, 1); ``eer`` / ``eer_threshold``: linear interpolation at the first k with far_k >= 1 - tar_k (NaN if none);
    ``tar_at_far``: per target, (the largest threshold with far_k <= target, its TAR) or None; ``best_accuracy`` / ``best_threshold``:
    the grid threshold that classifies the most pairs right (first of equals)."""
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    acc = np.asarray(accepted.cpu() if isinstance(accepted, torch.Tensor) else accepted, dtype=np.float64).reshape(2, -1)
    G, I = int(genuine_pairs), int(impostor_pairs)
    with np.errstate(invalid="ignore", divide="ignore"):
        tar = acc[0] / G if G else np.full(t.shape, np.nan)
        far = acc[1] / I if I else np.full(t.shape, np.nan)
    roc_auc = float(np.trapezoid(np.concatenate(([0.0], tar, [1.0])), np.concatenate(([0.0], far, [1.0])))) if G and I else float("nan")
    eer = eer_t = float("nan")
    if G and I:
        diff = far - (1.0 - tar)
        hit = np.nonzero(diff >= 0)[0]
        if hit.size:
            k = int(hit[0])
            if k == 0:
                eer, eer_t = float((far[0] + 1.0 - tar[0]) / 2), float(t[0])
            else:
                a = -diff[k - 1] / (diff[k] - diff[k - 1])
                eer = float((1.0 - tar[k - 1]) + a * ((1.0 - tar[k]) - (1.0 - tar[k - 1])))
                eer_t = float(t[k - 1] + a * (t[k] - t[k - 1]))
    tar_at_far = {}
    for f in far_targets:
        ok = np.nonzero(far <= f)[0] if I else np.zeros(0, np.int64)
        tar_at_far[f] = (float(t[ok[-1]]), float(tar[ok[-1]])) if ok.size else None
    total = G + I
    best_acc, best_t = float("nan"), float("nan")
    if total:
        right = acc[0] + (I - acc[1])
        kb = int(np.argmax(right))
        best_acc, best_t = float(right[kb] / total), float(t[kb])
    return {"thresholds": t, "genuine_pairs": G, "impostor_pairs": I, "tar": tar, "far": far, "roc_auc": roc_auc, "eer": eer,
            "eer_threshold": eer_t, "tar_at_far": tar_at_far, "best_accuracy": best_acc, "best_threshold": best_t}


def default_thresholds(emb: torch.Tensor, other: Optional[torch.Tensor] = None, n: int = 1024) -> np.ndarray:
    """``n`` fp32 thresholds evenly spaced on [0, 2 max ||row||_2 + 1e-3] (rows with a non-finite norm ignored), duplicates dropped:
    every finite pair distance lies inside.  One device reduction and one scalar copy."""
    rows = emb if other is None else torch.cat((emb.reshape(-1, emb.shape[-1]), other.reshape(-1, emb.shape[-1])))
    norms = torch.linalg.vector_norm(rows.to(torch.float32), dim=1) if rows.numel() else torch.zeros(1, device=rows.device)
    top = float(torch.where(torch.isfinite(norms), norms, torch.zeros_like(norms)).max()) if norms.numel() else 0.0
    return np.unique(np.linspace(0.0, 2.0 * top + 1e-3, n).astype(np.float32))


def verification_metrics(emb: torch.Tensor, labels, thresholds=None, other: Optional[torch.Tensor] = None, other_labels=None,
                         far_targets=FAR_TARGETS, prepared=None) -> dict:
    """The verification ROC of labelled embeddings, from EXACT pair counts on the GPU (`ops.verify_counts`): every unordered pair of
    ``emb`` (or, with ``other``, every pair of ``emb`` x ``other``) is genuine (same label) or impostor, accepted at t iff its distance
    ``||(a - b) + 1e-6||_2`` (the one `matching.search_batch` reports) is <= t.  Returns `metrics_from_counts`'s dict.  ``thresholds``:
    ascending, finite, >= 0, at most `ops.VERIFY_MAX_THRESHOLDS` (default: `default_thresholds`).  Sets of >= `ops.MATCH_MFMA_MIN_G`
    rows with D % 32 == 0 run on the MFMA path (packed here unless ``prepared`` is given)."""
    e = emb.to(torch.float32)
    dev = e.device
    la = torch.as_tensor(np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels, dtype=np.int32)).to(dev)
    b = lb = None
    if other is not None:
        b = other.to(device=dev, dtype=torch.float32)
        lb = torch.as_tensor(np.asarray(other_labels.cpu() if isinstance(other_labels, torch.Tensor) else other_labels,
                                        dtype=np.int32)).to(dev)
    if thresholds is None:
        thresholds = default_thresholds(e, b)
    t = np.asarray(thresholds.cpu() if isinstance(thresholds, torch.Tensor) else thresholds, dtype=np.float32).reshape(-1)
    target = e if b is None else b
    if prepared is None and ops.wants_pack(target.shape[0], target.shape[1]):
        target = target.contiguous()
        if b is None:
            e = target
        else:
            b = target
        prepared = ops.match_prepare(target)
    counts = ops.verify_counts(e, la, t, b, lb, prepared=prepared)
    G, I = pair_totals(la, lb)
    return metrics_from_counts(t, counts.cpu().numpy(), G, I, far_targets)


def evaluate_model(model, model_type: str, test_data, class_names: Optional[Sequence[str]] = None,
                   out_dir: Optional[str] = None, model_name: Optional[str] = None, dataset_name: str = "test",
                   batch_size: int = 32, arcface_classifier: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                   device="cuda") -> dict:
    """`src/testing.py:26-394` around the HIP path: batches of 32 → forward → softmax → arg-max → accumulate →
    sklearn metrics → the same JSON files.  What differs, by necessity: the model (already loaded, on the GPU, in
    ``eval()``) and the test set are passed in instead of being discovered under ``PROC_DATA_DIR`` / ``CHECKPOINTS_DIR``
    (`:29-129`, the reference's project layout and interactive prompt — out of scope), and the per-batch "inference
    time" is bracketed by device synchronisation (the reference's `time.time()` pair at `:164,255-273` times only the
    asynchronous launches on a GPU).

    ``test_data``: a directory in ``ImageFolder`` layout (class sub-folders; images are resized to 224×224 with PIL
    and normalised on the device), or an iterable of ready batches — ``(images fp32 NCHW, labels)``, for
    ``model_type == 'siamese'`` ``(img1, img2, labels)`` (`:170-182`; label 1 = same, prediction = distance < 0.5).
    ``arcface``: logits = cosine(embedding, class centres) (`:264-269`) unless ``arcface_classifier=(weight, bias)`` is
    given (the reference scores with a freshly initialised ``nn.Linear(512, C)``, `:134-136,262-263`).
    Returns the ``model_results`` dict (`:346-362`); with ``out_dir`` also writes ``<type>_model_results.json`` and
    ``experiment_summary.json`` (`:364-394`)."""
    import json
    import os
    import time
    if isinstance(test_data, (str, os.PathLike)):
        if model_type == 'siamese':
            raise ValueError("siamese evaluation takes an iterable of (img1, img2, labels) batches")
        samples, classes = image_folder(str(test_data))
        if not samples:
            raise FileNotFoundError(f"Found 0 files in subfolders of: {test_data}")
        class_names = list(classes) if class_names is None else list(class_names)
        batches = _folder_batches(samples, batch_size, device)
    else:
        batches = iter(test_data)
    if model.training:
        model.eval()                                                           # `:131`
    siamese = model_type == 'siamese'
    all_predictions, all_targets, all_probs, inference_times = [], [], [], []
    total_loss, nbatches = 0.0, 0
    with torch.no_grad():
        for batch in batches:
            if siamese:
                img1, img2, labels = batch
                img1, img2 = img1.to(device), img2.to(device)
                torch.cuda.synchronize()
                t0 = time.time()
                dist, same = siamese_verify(model, img1, img2, 0.5)             # `:175-177`
                torch.cuda.synchronize()
                inference_times.append(time.time() - t0)
                all_predictions.extend(same.cpu().numpy())
                all_targets.extend(np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels))
                all_probs.extend(dist.cpu().numpy()[:, None])                    # distances stand in for probabilities (`:182`)
                nbatches += 1
                continue
            images, labels = batch
            images = images.to(device)
            labels = torch.as_tensor(labels).to(torch.int64)
            torch.cuda.synchronize()
            t0 = time.time()
            if model_type == 'arcface':
                emb = model(images)
                if arcface_classifier is not None:
                    w, b = arcface_classifier
                    outputs = ops.linear_f32(emb, w.to(device).float(), None, None if b is None else b.to(device).float())
                else:
                    outputs, _ = ops.cosine_logits(emb, model.arcface.weight.detach(), s=1.0, want_argmax=False)
            else:
                outputs = model(images)
            torch.cuda.synchronize()
            inference_times.append(time.time() - t0)
            probs, pred = ops.softmax_argmax(outputs)                           # `:278-279`
            logits = outputs.float().cpu()
            lse = torch.logsumexp(logits, dim=1)
            total_loss += float((lse - logits[torch.arange(logits.shape[0]), labels]).mean())   # nn.CrossEntropyLoss, `:275-276`
            nbatches += 1
            all_predictions.extend(pred.cpu().numpy())
            all_targets.extend(labels.numpy())
            all_probs.extend(probs.cpu().numpy())
    if nbatches == 0:
        raise ValueError("evaluate_model: the test set is empty")
    all_predictions, all_targets, all_probs = np.array(all_predictions), np.array(all_targets), np.array(all_probs)
    metrics = classification_metrics(all_targets, all_predictions, all_probs, siamese)
    metrics["inference_time"] = float(np.mean(inference_times))                # `:315`
    if siamese:
        class_names = ['Same', 'Different']                                     # `:330`
    elif class_names is None:
        class_names = [str(i) for i in range(all_probs.shape[1])]
    model_results = {"predictions": all_predictions.tolist(), "targets": all_targets.tolist(),
                     "probabilities": all_probs.tolist(), "class_names": list(class_names), "metrics": metrics}
    if not siamese:
        model_results["test_loss"] = total_loss / nbatches                      # printed at `:327`
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, _results_file_name(model_type)), 'w') as f:
            json.dump(model_results, f, indent=2)
        with open(os.path.join(out_dir, 'experiment_summary.json'), 'w') as f:   # `:384-394`
            json.dump({"model_type": model_type, "model_name": model_name or model_type, "dataset": dataset_name,
                       "metrics": metrics, "class_names": list(class_names)}, f, indent=2)
    return model_results


# ------------------------------------------------------------------------------------------------
# The classification tally: the accumulate step of `src/testing.py:278-283` and the metric block of `src/advanced_metrics.py`
# (per-class precision / recall / F1, the enhanced confusion matrix, expected / maximum calibration error) from exact integers
# kept on the device (`ops.classify_tally`), as `verification_metrics` does for pairs.  The rule below is the specification; its
# integer half is csrc/tally_rule.h, which the kernel and its host twin compile.
# ------------------------------------------------------------------------------------------------
TALLY_HEADER_WORDS = 8
TALLY_LOSS_CLAMP, TALLY_LOSS_SCALE, TALLY_CONF_SCALE = 65536.0, float(2 ** 24), float(2 ** 32)


def tally_layout(C: int, ranks: int = 6, n_bins: int = 10, confusion: bool = True) -> dict:
    """name -> slice of the uint64 state: an 8-word header (``rows, ignored, nonfinite, correct, loss_q``, three reserved zero
    words), then ``rank_hist`` [ranks], ``support`` / ``predicted`` / ``hit`` [C], ``bin_count`` / ``bin_correct`` / ``bin_conf_q``
    [n_bins] and, when kept, ``confusion`` [C * C] (row = label, column = prediction).  ``"words"`` -> the total."""
    out = {name: slice(k, k + 1) for k, name in enumerate(ops.TALLY_HEADER)}
    at = TALLY_HEADER_WORDS
    for name, n in [("rank_hist", ranks), ("support", C), ("predicted", C), ("hit", C), ("bin_count", n_bins), ("bin_correct", n_bins),
                    ("bin_conf_q", n_bins)] + ([("confusion", C * C)] if confusion else []):
        out[name] = slice(at, at + int(n))
        at += int(n)
    out["words"] = at
    return out


def tally_edges(n_bins: int) -> np.ndarray:
    """The bin edges as the kernel forms them: ``edge_k = k * (1 / (n_bins - 1))`` in float64, the last one 1.0, the single edge of
    ``n_bins == 1`` 0 - bit for bit ``np.linspace(0, 1, n_bins)`` for n_bins 1 ... 1024 (tested)."""
    if n_bins == 1:
        return np.zeros(1, np.float64)
    e = np.arange(n_bins, dtype=np.float64) * (1.0 / float(n_bins - 1))
    e[-1] = 1.0
    return e


def tally_row_rule(logits, labels):
    """The integer half of the row rule: ``(pred int32, rank int32, why int8)`` per row.  ``why`` 1: the label is outside
    ``[0, C)`` - the row is ignored whatever its logits are; 2: a logit is NaN or infinite; 0: counted.  Declined rows have
    pred = rank = -1.  ``pred`` is the first arg-max; ``rank = #{c : z[c] > z[y]} + #{c < y : z[c] == z[y]}``, so rank == 0 iff
    pred == y.  fp32 comparisons only: exact on any machine."""
    z = np.asarray(logits, dtype=np.float32)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    B, C = z.shape
    why = np.zeros(B, np.int8)
    why[(y < 0) | (y >= C)] = 1
    why[(why == 0) & ~np.isfinite(z).all(axis=1)] = 2
    pred, rank = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    ok = why == 0
    if ok.any():
        zc, yc = z[ok], y[ok]
        zy = zc[np.arange(len(yc)), yc][:, None]
        pred[ok] = zc.argmax(axis=1)                                           # (numpy's arg-max is the first one)
        rank[ok] = (zc > zy).sum(axis=1) + ((zc == zy) & (np.arange(C)[None, :] < yc[:, None])).sum(axis=1)
    return pred, rank, why


def tally_rows_reference(logits, labels):
    """The row records in float64: ``(pred, rank, conf, loss)`` with ``conf = 1 / sum_c exp(z[c] - z[pred])`` and
    ``loss = max(0, log sum_c exp(z[c] - z[pred]) + (z[pred] - z[y]))`` (NaN for declined rows) - what the kernel's fp32 values
    are measured against."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    pred, rank, why = tally_row_rule(logits, labels)
    conf, loss = np.full(len(y), np.nan), np.full(len(y), np.nan)
    ok = why == 0
    if ok.any():
        zc, yc = z[ok], y[ok]
        mx = zc.max(axis=1)
        s = np.exp(zc - mx[:, None]).sum(axis=1)
        conf[ok] = 1.0 / s
        loss[ok] = np.maximum(0.0, np.log(s) + (mx - zc[np.arange(len(yc)), yc]))
    return pred, rank, conf, loss


def tally_rule(logits, labels, row_conf, row_loss, ranks: int = 6, n_bins: int = 10, confusion: bool = True, state=None):
    """THE ACCUMULATION RULE in numpy: add the rows to a uint64 state (a fresh one if ``state`` is None) and return
    ``(state, pred, rank)``.  ``row_conf`` / ``row_loss`` are the rows' fp32 confidence and loss (the device's own values: the
    rule is defined on their bits); pred and rank come from `tally_row_rule`.

    A declined row adds 1 to ``ignored`` (label outside [0, C)) or ``nonfinite`` and nothing else.  A counted row adds:
    ``rows += 1``, ``correct += (rank == 0)``, ``loss_q += rint(min(float64(loss), 65536) * 2^24)``;
    ``rank_hist[min(rank, ranks - 1)] += 1``; ``support[y] += 1``, ``predicted[pred] += 1``, ``hit[y] += (rank == 0)``; with
    ``b = np.digitize(float64(conf), tally_edges(n_bins)) - 1`` (the reference's rule: n_bins EDGES, so only conf == 1.0 reaches
    the last bin) ``bin_count[b] += 1``, ``bin_correct[b] += (rank == 0)``, ``bin_conf_q[b] += rint(float64(conf) * 2^32)``; and
    ``confusion[y * C + pred] += 1`` where the matrix is kept.  Integers only: the state does not depend on the order of the rows
    or on how they are split into calls.  ``loss_q`` overflows after 2^24 rows at the clamp, 2^34 rows of losses below 64."""
    z = np.asarray(logits, dtype=np.float32)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    B, C = z.shape
    conf = np.asarray(row_conf, dtype=np.float32).astype(np.float64).reshape(-1)
    loss = np.asarray(row_loss, dtype=np.float32).astype(np.float64).reshape(-1)
    lay = tally_layout(C, ranks, n_bins, confusion)
    if state is None:
        state = np.zeros(lay["words"], np.uint64)
    assert state.dtype == np.uint64 and state.shape == (lay["words"],)
    pred, rank, why = tally_row_rule(z, y)
    ok = why == 0
    one = np.uint64(1)
    state[1] += np.uint64(int((why == 1).sum()))
    state[2] += np.uint64(int((why == 2).sum()))
    yc, pc, rc, cc, lc = y[ok], pred[ok].astype(np.int64), rank[ok].astype(np.int64), conf[ok], loss[ok]
    right = (rc == 0).astype(np.uint64)
    state[0] += np.uint64(len(yc))
    state[3] += np.uint64(int(right.sum()))
    state[4] += np.rint(np.minimum(lc, TALLY_LOSS_CLAMP) * TALLY_LOSS_SCALE).astype(np.uint64).sum(dtype=np.uint64)
    b = np.digitize(cc, tally_edges(n_bins)) - 1
    np.add.at(state, lay["rank_hist"].start + np.minimum(rc, ranks - 1), one)
    np.add.at(state, lay["support"].start + yc, one)
    np.add.at(state, lay["predicted"].start + pc, one)
    np.add.at(state, lay["hit"].start + yc, right)
    np.add.at(state, lay["bin_count"].start + b, one)
    np.add.at(state, lay["bin_correct"].start + b, right)
    np.add.at(state, lay["bin_conf_q"].start + b, np.rint(cc * TALLY_CONF_SCALE).astype(np.uint64))
    if confusion:
        np.add.at(state, lay["confusion"].start + yc * C + pc, one)
    return state, pred, rank


def tally_counts(state, C: int, ranks: int = 6, n_bins: int = 10, confusion: bool = True) -> dict:
    """A state (uint64 / int64 words, numpy) as integers by name: the five header counters as Python ints, ``rank_hist``,
    ``support``, ``predicted``, ``hit``, ``bin_count``, ``bin_correct`` as int64 arrays, ``bin_conf_q`` as uint64 and
    ``confusion`` as an int64 ``[C, C]`` matrix (row = label, column = prediction) or None where it is not kept."""
    a = np.ascontiguousarray(state).view(np.uint64).reshape(-1)
    lay = tally_layout(C, ranks, n_bins, confusion)
    if a.size != lay["words"]:
        raise ValueError(f"tally_counts: {a.size} words, C = {C}, ranks = {ranks}, n_bins = {n_bins}, confusion = {confusion} have {lay['words']}")
    out = {name: int(a[k]) for k, name in enumerate(ops.TALLY_HEADER)}
    for name in ("rank_hist", "support", "predicted", "hit", "bin_count", "bin_correct"):
        out[name] = a[lay[name]].astype(np.int64)
    out["bin_conf_q"] = a[lay["bin_conf_q"]].copy()
    out["confusion"] = a[lay["confusion"]].astype(np.int64).reshape(C, C) if confusion else None
    return out


def metrics_from_tally(counts: dict, class_names: Optional[Sequence[str]] = None) -> dict:
    """Float64 metrics from the integers of a tally (`tally_counts` / `ClassificationTally.counts`).  With no counted row every
    ratio over the rows is NaN; nothing raises.

    * ``accuracy`` = correct / rows; ``precision`` / ``recall`` / ``f1``: sklearn's ``average='weighted'`` with ``zero_division=0``
      (per class hit / predicted, hit / support, 2 hit / (predicted + support), 0 where the denominator is 0; weights = support);
    * ``top_k``: ``{k: fraction of rows with rank < k}`` for 1 <= k < ranks (the last cell of the rank histogram pools every rank
      from ranks - 1 on);
    * ``loss``: the PER-SAMPLE mean of the fp32 row losses (from the 2^-24 fixed point).  `evaluate_model`'s ``test_loss`` is the
      mean of the batch means (`testing.py:275-276,327`): the two differ when the last batch is short;
    * ``per_class``: `advanced_metrics.calculate_per_class_metrics`'s fields except ``roc_auc``, which is no function of these
      counts (`ovr_metrics` gives it, and `evaluate_stream(auc=True)` puts it here), for
      every class 0 ... C - 1 (the reference, through sklearn, numbers only the classes that occur in the labels or predictions);
    * ``confusion``: `advanced_metrics.create_enhanced_confusion_matrix`'s dict (``misclassified_to``: the top 3 by fraction,
      ties in class order), None where the matrix was not kept;
    * ``calibration``: `advanced_metrics.expected_calibration_error`'s dict - empty bins read 0, the ECE weights are
      bin_count / rows, the MCE is the maximum over all bins;
    * ``rows`` / ``ignored`` / ``nonfinite``: the counted and the declined rows."""
    support = np.asarray(counts["support"], dtype=np.float64)
    predicted = np.asarray(counts["predicted"], dtype=np.float64)
    hit = np.asarray(counts["hit"], dtype=np.float64)
    C, rows = len(support), int(counts["rows"])
    names = [str(i) for i in range(C)] if class_names is None else list(class_names)
    nan = float("nan")

    def ratio(num, den):
        return np.divide(num, den, out=np.zeros_like(num, dtype=np.float64), where=den > 0)
    prec, rec, f1 = ratio(hit, predicted), ratio(hit, support), ratio(2.0 * hit, predicted + support)
    total = float(support.sum())
    weighted = (lambda v: float((v * support).sum() / total)) if rows else (lambda v: nan)
    rank_hist = np.asarray(counts["rank_hist"], dtype=np.int64)
    m = {"rows": rows, "ignored": int(counts["ignored"]), "nonfinite": int(counts["nonfinite"]),
         "accuracy": int(counts["correct"]) / rows if rows else nan,
         "precision": weighted(prec), "recall": weighted(rec), "f1": weighted(f1),
         "top_k": {k: (int(rank_hist[:k].sum()) / rows if rows else nan) for k in range(1, len(rank_hist))},
         "loss": int(counts["loss_q"]) / TALLY_LOSS_SCALE / rows if rows else nan}
    m["per_class"] = {names[i]: {"precision": float(prec[i]), "recall": float(rec[i]), "f1": float(f1[i]), "support": int(support[i]),
                                 "accuracy": float(rec[i])} for i in range(min(C, len(names)))}
    cm = counts.get("confusion")
    if cm is None:
        m["confusion"] = None
    else:
        cm = np.asarray(cm, dtype=np.int64).reshape(C, C)
        rows_total, cols_total = cm.sum(axis=1), cm.sum(axis=0)
        info = {}
        for i in range(min(C, len(names))):
            tp = int(cm[i, i])
            mis = [(names[j], float(cm[i, j] / rows_total[i])) for j in range(min(C, len(names))) if j != i and cm[i, j] > 0] if rows_total[i] > 0 else []
            mis.sort(key=lambda x: x[1], reverse=True)                         # (stable: ties stay in class order)
            info[names[i]] = {"true_positives": tp, "false_positives": int(cols_total[i]) - tp, "false_negatives": int(rows_total[i]) - tp,
                              "precision": float(tp / cols_total[i]) if cols_total[i] > 0 else 0.0,
                              "recall": float(tp / rows_total[i]) if rows_total[i] > 0 else 0.0,
                              "support": int(rows_total[i]), "misclassified_to": mis[:3]}
        m["confusion"] = {"matrix": cm.tolist(), "class_names": names, "class_statistics": info}
    bc = np.asarray(counts["bin_count"], dtype=np.float64)
    acc_b = ratio(np.asarray(counts["bin_correct"], dtype=np.float64), bc)
    conf_b = ratio(np.asarray(counts["bin_conf_q"]).astype(np.float64) / TALLY_CONF_SCALE, bc)
    gap = np.abs(acc_b - conf_b)
    m["calibration"] = {"expected_calibration_error": float((gap * (bc / rows)).sum()) if rows else nan,
                        "maximum_calibration_error": float(gap.max()), "bin_accuracies": acc_b.tolist(),
                        "bin_confidences": conf_b.tolist(), "bin_counts": bc.tolist(), "n_bins": len(bc)}
    return m


class ClassificationTally:
    """A device-resident classification tally: `update` adds a batch of logits and labels in one launch (`ops.classify_tally`) with
    no copy and no synchronisation, `counts` / `metrics` make the one device-to-host copy at the end.  ``confusion=None`` keeps the
    confusion matrix when ``num_classes <= 2048`` (32 MiB of state at most)."""

    def __init__(self, num_classes: int, ranks: int = 6, n_bins: int = 10, confusion: Optional[bool] = None, device="cuda"):
        self.num_classes, self.ranks, self.n_bins = int(num_classes), int(ranks), int(n_bins)
        self.confusion = self.num_classes <= 2048 if confusion is None else bool(confusion)
        self.layout = ops.classify_tally_layout(self.num_classes, self.ranks, self.n_bins, self.confusion)   # (refuses a bad shape)
        self.state = torch.zeros((ops.classify_tally_words(self.num_classes, self.ranks, self.n_bins, self.confusion),),
                                 dtype=torch.int64, device=device)

    def _shape(self):
        return self.num_classes, self.ranks, self.n_bins, self.confusion

    def update(self, logits: torch.Tensor, labels) -> "ClassificationTally":
        """Add ``logits`` float32 ``[B, C]`` (on the tally's device) and ``labels`` ``[B]`` (any integer tensor or sequence; a
        label outside ``[0, C)`` declines its row).  No synchronisation; an empty batch is a no-op."""
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"ClassificationTally.update: logits {tuple(logits.shape)} for {self.num_classes} classes")
        if logits.shape[0] == 0:
            return self
        labels = torch.as_tensor(labels)
        if labels.dtype != torch.int32:                                        # (a wide label must not wrap into the range)
            labels = labels.to(torch.int64).clamp(-1, self.num_classes).to(torch.int32)
        ops.classify_tally(logits, labels.to(self.state.device, non_blocking=True), self.state, self.ranks, self.n_bins, self.confusion)
        return self

    def merge(self, other: "ClassificationTally") -> "ClassificationTally":
        """Integer add of another tally with the same layout (another rank's, another shard's): the result is the tally of the
        rows of both, whatever their order."""
        if self._shape() != other._shape():
            raise ValueError(f"ClassificationTally.merge: layouts differ ({self._shape()} and {other._shape()})")
        self.state += other.state.to(self.state.device)
        return self

    def reset(self) -> "ClassificationTally":
        self.state.zero_()
        return self

    def counts(self) -> dict:
        """The one device-to-host copy: the integers by name (`tally_counts`)."""
        return tally_counts(self.state.cpu().numpy(), *self._shape())

    def metrics(self, class_names: Optional[Sequence[str]] = None) -> dict:
        return metrics_from_tally(self.counts(), class_names)


def evaluate_stream(model, model_type: str, test_data, num_classes: Optional[int] = None, class_names: Optional[Sequence[str]] = None,
                    batch_size: int = 32, ranks: int = 6, n_bins: int = 10,
                    arcface_classifier: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, device="cuda", auc: bool = False) -> dict:
    """The loop of `evaluate_model` with a `ClassificationTally` in place of the host lists: every batch is forward -> one
    `ops.classify_tally` launch, nothing is copied back and nothing waits until the single synchronisation at the end.
    ``test_data``, ``arcface_classifier`` and the arcface logits (cosine against the class centres, or the given classifier) are
    `evaluate_model`'s; ``num_classes`` defaults to the width of the first batch's logits.  Returns `metrics_from_tally`'s dict.
    ``auc=True`` adds the one-vs-rest ROC AUC and average precision of `evaluate_model`'s metric block: every batch then also runs
    `ops.softmax_argmax` and appends the probabilities - the bits `evaluate_model` copies to the host - to an `OvrScores` store on
    the device (two more launches a batch, still no copy and no wait; the store's capacity is the folder's sample count where that
    is known), and the returned dict gains ``roc_auc`` and ``pr_auc`` (`ovr_metrics`: NaN where a class has no sample, as
    `evaluate_model` reports) and ``roc_auc`` / ``average_precision`` inside every ``per_class`` entry.  The store declines a row
    on its probabilities, the tally on its logits: a row with a -inf logit has finite probabilities and is counted by the store
    alone.  ``auc=False``: no extra launch, the same dict as ever.  `evaluate_model` remains the way to the reference's JSON files.
    ``model_type == 'siamese'`` raises ``ValueError`` (pairs are `verification_metrics`' business)."""
    import os
    if model_type == 'siamese':
        raise ValueError("evaluate_stream tallies classifications; siamese pairs go through evaluate_model or verification_metrics")
    known_rows = None
    if isinstance(test_data, (str, os.PathLike)):
        samples, classes = image_folder(str(test_data))
        if not samples:
            raise FileNotFoundError(f"Found 0 files in subfolders of: {test_data}")
        class_names = list(classes) if class_names is None else list(class_names)
        batches = _folder_batches(samples, batch_size, device)
        known_rows = len(samples)
    else:
        batches = iter(test_data)
    if model.training:
        model.eval()
    tally = ovr = None
    with torch.no_grad():
        for images, labels in batches:
            images = images.to(device)
            if model_type == 'arcface':
                emb = model(images)
                if arcface_classifier is not None:
                    w, b = arcface_classifier
                    outputs = ops.linear_f32(emb, w.to(device).float(), None, None if b is None else b.to(device).float())
                else:
                    outputs, _ = ops.cosine_logits(emb, model.arcface.weight.detach(), s=1.0, want_argmax=False)
            else:
                outputs = model(images)
            outputs = outputs.float()
            if tally is None:
                tally = ClassificationTally(int(outputs.shape[1]) if num_classes is None else int(num_classes), ranks, n_bins,
                                            device=outputs.device)
            tally.update(outputs, labels)
            if auc:
                if ovr is None:
                    ovr = OvrScores(tally.num_classes, OVR_DEFAULT_CAPACITY if known_rows is None else known_rows, device=outputs.device)
                ovr.update(ops.softmax_argmax(outputs)[0], labels)
    if tally is None:
        raise ValueError("evaluate_stream: the test set is empty")
    m = tally.metrics(class_names)                                             # the one synchronisation: the state's copy to the host
    if auc:
        o = ovr.metrics(class_names)                                           # (and the one copy of the counts)
        m["roc_auc"], m["pr_auc"] = o["roc_auc"], o["pr_auc"]
        for name, entry in m["per_class"].items():
            entry["roc_auc"], entry["average_precision"] = o["per_class"][name]["roc_auc"], o["per_class"][name]["average_precision"]
    return m


# ------------------------------------------------------------------------------------------------
# One-vs-rest ROC AUC and average precision (`src/testing.py:296-312`: ``roc_auc_score(multi_class='ovr')`` and
# ``average_precision_score``; the per-class ``roc_auc`` of `src/advanced_metrics.py:85-100`) without a sort and without the
# scores on the host.  Every counted row is a positive of exactly one class, its own label; three integers per row - how many
# rows of its class, and of the other classes, score at least as high in that class's column, and how many of the others tie
# with it - decide both curves for that class.  The device keeps the scores (`OvrScores`, `ops.ovr_append`) and counts the pairs
# (`ops.ovr_rank_counts`); the rule below is the specification, csrc/ovr_rule.h what the kernel and its host twin compile.
# ------------------------------------------------------------------------------------------------
OVR_DEFAULT_CAPACITY = 4096


def ovr_stored_labels(scores, labels) -> np.ndarray:
    """The label a score store keeps for each row of ``scores`` ``[N, C]``: the label if it lies in ``[0, C)`` and every score of
    the row is finite; -1 for a label outside the range, whatever the scores are; -2 for a NaN or an infinity under a valid label
    (the tally's two kinds of declined row)."""
    z = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    out = np.where((y < 0) | (y >= z.shape[1]), -1, y)
    out[(out >= 0) & ~np.isfinite(z).all(axis=1)] = -2
    return out.astype(np.int32)


def ovr_rank_rule(scores, labels):
    """THE COUNTING RULE in numpy, on ``scores`` float32 ``[N, C]`` (row-major) and ``labels`` ``[N]``: returns
    ``(ge_same, ge_other, eq_other, why)``, three uint64 ``[N]`` arrays and an int8 one.  ``why`` 1: the label is outside
    ``[0, C)`` (a stored -1 or -2 lands here too); 2: a score of the row is NaN or infinite; 0: counted.  For a counted row i with
    label y_i and ``s_i = scores[i, y_i]``, over the counted rows j (j == i included):

    * ``ge_same[i]``  = #{j : y_j == y_i and scores[j, y_i] >= s_i} (so >= 1),
    * ``ge_other[i]`` = #{j : y_j != y_i and scores[j, y_i] >= s_i},
    * ``eq_other[i]`` = #{j : y_j != y_i and scores[j, y_i] == s_i}.

    A declined row gets 0, 0, 0 and takes part in nobody's count.  fp32 IEEE comparisons (-0.0 equals +0.0, a denormal is not
    zero): exact integers that do not depend on the order of the rows or on how they were split into appends."""
    z = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    N, C = z.shape
    why = np.zeros(N, np.int8)
    why[(y < 0) | (y >= C)] = 1
    why[(why == 0) & ~np.isfinite(z).all(axis=1)] = 2
    ok = why == 0
    ge_same, ge_other, eq_other = (np.zeros(N, np.uint64) for _ in range(3))
    for c in np.unique(y[ok]):
        pos = np.nonzero(ok & (y == c))[0]
        same, other = z[pos, c], z[ok & (y != c), c]
        for lo in range(0, len(pos), 1024):                                   # (1024 positives at a time bound the temporaries)
            s = same[lo:lo + 1024, None]
            ge_same[pos[lo:lo + 1024]] = (same[None, :] >= s).sum(axis=1)
            ge_other[pos[lo:lo + 1024]] = (other[None, :] >= s).sum(axis=1)
            eq_other[pos[lo:lo + 1024]] = (other[None, :] == s).sum(axis=1)
    return ge_same, ge_other, eq_other, why


def ovr_metrics(labels, ge_same, ge_other, eq_other, num_classes: int, class_names: Optional[Sequence[str]] = None) -> dict:
    """Float64 one-vs-rest metrics from the integers of `ovr_rank_rule` / `ops.ovr_rank_counts` and the STORED labels
    (`ovr_stored_labels`: -1 ignored, -2 non-finite; any other value outside ``[0, num_classes)`` reads as ignored).  With P_c
    positives and N_c = rows - P_c negatives of class c:

    * ``roc_auc[c] = (sum_i (N_c - ge_other[i]) + 1/2 sum_i eq_other[i]) / (P_c N_c)`` over the positives i of c - the
      Mann-Whitney form of the trapezoid under ``roc_curve``, ties at one half - NaN if P_c == 0 or N_c == 0.  Both sums are
      integers; the quotient is rounded once;
    * ``average_precision[c] = (sum_i ge_same[i] / (ge_same[i] + ge_other[i])) / P_c`` - sklearn's step-wise sum: positives that
      share a threshold each contribute that threshold's precision - NaN if P_c == 0.  The sum runs in row order.

    Returns ``per_class`` ``{name: {roc_auc, average_precision, support}}`` for every class 0 ... C - 1, ``roc_auc`` and ``pr_auc``,
    the plain means over all C classes - ``roc_auc_score(multi_class='ovr')`` and the multiclass ``average_precision_score`` - each
    NaN as soon as one class has no defined value (sklearn raises there, and `evaluate_model` reports NaN), and ``rows`` /
    ``ignored`` / ``nonfinite``."""
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    C = int(num_classes)
    a, b, e = (np.asarray(v).reshape(-1).astype(np.uint64) for v in (ge_same, ge_other, eq_other))   # (int64 words wrap back)
    if not (len(a) == len(b) == len(e) == len(y)):
        raise ValueError(f"ovr_metrics: {len(y)} labels and {len(a)}, {len(b)}, {len(e)} counts")
    names = [str(i) for i in range(C)] if class_names is None else list(class_names)
    counted = np.nonzero((y >= 0) & (y < C))[0]
    rows, nonfinite = len(counted), int((y == -2).sum())
    order = counted[np.argsort(y[counted], kind="stable")]                    # by class, in row order inside a class
    support = np.bincount(y[counted], minlength=C)
    ends = np.cumsum(support)
    nan = float("nan")
    roc, ap = np.full(C, nan), np.full(C, nan)
    for c in range(C):
        P, Nn = int(support[c]), rows - int(support[c])
        if P == 0:
            continue
        i = order[ends[c] - P: ends[c]]
        ga, gb = a[i].astype(np.float64), b[i].astype(np.float64)
        ap[c] = float(np.cumsum(ga / (ga + gb))[-1]) / P                      # (cumsum adds in order)
        if Nn:
            below = P * Nn - int(b[i].sum(dtype=np.uint64))                   # (integer sums, each at most P_c N_c)
            roc[c] = (2 * below + int(e[i].sum(dtype=np.uint64))) / (2 * P * Nn)   # (Python integers: one rounding)
    per_class = {names[c]: {"roc_auc": float(roc[c]), "average_precision": float(ap[c]), "support": int(support[c])}
                 for c in range(min(C, len(names)))}
    return {"rows": rows, "ignored": len(y) - rows - nonfinite, "nonfinite": nonfinite, "per_class": per_class,
            "roc_auc": float(np.cumsum(roc)[-1] / C) if C and not np.isnan(roc).any() else nan,
            "pr_auc": float(np.cumsum(ap)[-1] / C) if C and not np.isnan(ap).any() else nan}


class OvrScores:
    """A device-resident score store: `update` appends a batch of scores and labels in one launch (`ops.ovr_append`) with no copy
    to the host and no synchronisation; `rank_counts` / `metrics` run the one count (`ops.ovr_rank_counts`) and make the one
    device-to-host copy at the end.  The store is ``[num_classes, capacity]`` float32, class-major; past the capacity it grows by
    doubling, with a device copy of the rows held.  4 ``num_classes`` bytes per row: 100 000 rows of 36 classes are 14 MB, of
    10 000 classes 4 GB."""

    def __init__(self, num_classes: int, capacity: int = OVR_DEFAULT_CAPACITY, device="cuda"):
        self.num_classes, self.rows = int(num_classes), 0
        if self.num_classes < 1 or int(capacity) < 1:
            raise ValueError(f"OvrScores: num_classes = {num_classes} and capacity = {capacity} must be at least 1")
        self.store = torch.empty((self.num_classes, int(capacity)), dtype=torch.float32, device=device)
        self.labels = torch.empty((int(capacity),), dtype=torch.int32, device=device)

    @property
    def capacity(self) -> int:
        return int(self.labels.shape[0])

    def _reserve(self, rows: int) -> None:
        if rows <= self.capacity:
            return
        cap = max(2 * self.capacity, rows)
        store = torch.empty((self.num_classes, cap), dtype=torch.float32, device=self.store.device)
        labels = torch.empty((cap,), dtype=torch.int32, device=self.store.device)
        store[:, :self.rows] = self.store[:, :self.rows]
        labels[:self.rows] = self.labels[:self.rows]
        self.store, self.labels = store, labels

    def update(self, scores: torch.Tensor, labels) -> "OvrScores":
        """Append ``scores`` float32 ``[B, C]`` (on the store's device) and ``labels`` ``[B]`` (any integer tensor or sequence; a
        label outside ``[0, C)`` declines its row, and so does a non-finite score).  No synchronisation; an empty batch is a no-op."""
        if scores.dim() != 2 or scores.shape[1] != self.num_classes:
            raise ValueError(f"OvrScores.update: scores {tuple(scores.shape)} for {self.num_classes} classes")
        B = int(scores.shape[0])
        if B == 0:
            return self
        labels = torch.as_tensor(labels)
        if labels.dtype != torch.int32:                                        # (a wide label must not wrap into the range)
            labels = labels.to(torch.int64).clamp(-1, self.num_classes).to(torch.int32)
        self._reserve(self.rows + B)
        ops.ovr_append(scores, labels.to(self.store.device, non_blocking=True), self.store, self.labels, self.rows)
        self.rows += B
        return self

    def merge(self, other: "OvrScores") -> "OvrScores":
        """The rows of both, this store's first (another rank's or another shard's store; a device copy)."""
        if other.num_classes != self.num_classes:
            raise ValueError(f"OvrScores.merge: {self.num_classes} and {other.num_classes} classes")
        n = other.rows
        self._reserve(self.rows + n)
        self.store[:, self.rows:self.rows + n] = other.store[:, :n].to(self.store.device)
        self.labels[self.rows:self.rows + n] = other.labels[:n].to(self.store.device)
        self.rows += n
        return self

    def reset(self) -> "OvrScores":
        self.rows = 0
        return self

    def rank_counts(self):
        """One count and the one device-to-host copy: ``(stored labels int32, ge_same, ge_other, eq_other uint64)`` of the rows held."""
        if self.rows == 0:
            return (np.zeros(0, np.int32),) + tuple(np.zeros(0, np.uint64) for _ in range(3))
        counts = ops.ovr_rank_counts(self.store, self.labels, self.rows)
        host = torch.stack((self.labels[:self.rows].to(torch.int64),) + tuple(counts)).cpu().numpy()
        return (host[0].astype(np.int32),) + tuple(host[k].view(np.uint64) for k in (1, 2, 3))

    def metrics(self, class_names: Optional[Sequence[str]] = None) -> dict:
        return ovr_metrics(*self.rank_counts(), self.num_classes, class_names)


# ------------------------------------------------------------------------------------------------
# `src/testing.py:532-595`: predict_image
# ------------------------------------------------------------------------------------------------
def predict_image(model_type: str, image_path: str, model_name: Optional[str] = None, checkpoints_dir: str = "outputs/checkpoints",
                  proc_data_dir: str = "data/processed", device="cuda") -> Tuple[str, float]:
    """Make a prediction for a single image: ``(class_name, probability)`` - `src/testing.py:532-595` on the HIP path.

    Same discovery rules and errors as the reference: the latest ``<model_type>_*`` directory under ``checkpoints_dir``
    (``CHECKPOINTS_DIR``, `base_config.py:18`) unless ``model_name`` is given; class names from ``ImageFolder(<first processed
    dataset>/train)`` under ``proc_data_dir`` (``PROC_DATA_DIR``, `base_config.py:15`); ``best_model.pth`` before
    ``best_checkpoint.pth``; ``'siamese'`` is refused.  The image is resized to 224x224 on the device (bit-exact with the PIL
    bilinear ``transforms.Resize``), ToTensor + Normalize run inside the stem, then forward -> softmax -> max.
    Checkpoints are read with ``weights_only=True`` (a ``state_dict`` of tensors; nothing in the file is executed)."""
    import os
    from pathlib import Path
    from PIL import Image
    from .face_models import get_model
    ckpt_root, proc_root = Path(checkpoints_dir), Path(proc_data_dir)
    if model_name is None:
        model_dirs = list(ckpt_root.glob(f'{model_type}_*'))
        if not model_dirs:
            raise ValueError(f"No trained models found for type: {model_type}")
        model_name = sorted(model_dirs)[-1].name
    model_checkpoint_dir = ckpt_root / model_name
    if not model_checkpoint_dir.exists():
        raise ValueError(f"Model not found: {model_name}")
    processed_dirs = [d for d in proc_root.iterdir() if d.is_dir() and (d / "train").exists()] if proc_root.exists() else []
    if not processed_dirs:
        raise ValueError("No processed datasets found.")
    if model_type == 'siamese':
        raise ValueError("Siamese model can't be used for direct prediction. Use it for verification.")
    classes = sorted(d.name for d in os.scandir(processed_dirs[0] / "train") if d.is_dir())   # ImageFolder(...).classes
    with Image.open(image_path) as im:
        u8 = resize_to_u8([im.convert('RGB')], (224, 224), device=device)                    # uint8 [1, 224, 224, 3] on the device
    model = get_model(model_type, num_classes=len(classes)).to(device)
    best_model_path, best_checkpoint_path = model_checkpoint_dir / 'best_model.pth', model_checkpoint_dir / 'best_checkpoint.pth'
    if best_model_path.exists():
        model.load_state_dict(torch.load(best_model_path, map_location=device, weights_only=True))
    elif best_checkpoint_path.exists():
        model.load_state_dict(torch.load(best_checkpoint_path, map_location=device, weights_only=True))
    else:
        raise FileNotFoundError(f"Neither best_model.pth nor best_checkpoint.pth found in {model_checkpoint_dir}")
    model.eval()
    with torch.no_grad():
        x = u8 if getattr(model, "supports_u8_input", False) else preprocess(u8, IMAGENET_MEAN, IMAGENET_STD, device)
        outputs = model(x)
        probs, pred = ops.softmax_argmax(outputs)
        pred_idx = int(pred[0])
        return classes[pred_idx], float(probs[0, pred_idx])


# ------------------------------------------------------------------------------------------------
# `src/testing.py:26-131`: the discovery half of the reference's evaluate_model (which checkpoint, which processed dataset)
# ------------------------------------------------------------------------------------------------
def find_processed_datasets(proc_data_dir: str):
    """`testing.py:43-70`: ``[(path, display name)]`` of the processed datasets that hold a ``test`` split - ``<config>/test``,
    ``<config>/<dataset>/test`` and the root's own ``test``, in the reference's order, de-duplicated by display name."""
    from pathlib import Path
    root = Path(proc_data_dir)
    found, names = [], set()
    if not root.exists():
        return found
    for config_dir in [d for d in root.iterdir() if d.is_dir() and d.name not in ["train", "val", "test"]]:
        if (config_dir / "test").exists():
            if config_dir.name not in names:
                found.append((config_dir, config_dir.name)); names.add(config_dir.name)
        else:
            for dataset_dir in config_dir.iterdir():
                if dataset_dir.is_dir() and (dataset_dir / "test").exists():
                    disp = f"{config_dir.name}/{dataset_dir.name}"
                    if disp not in names:
                        found.append((dataset_dir, disp)); names.add(disp)
    if (root / "test").exists() and "root" not in names:
        found.append((root, "processed (root)"))
    return found


def evaluate_trained(model_type: str, model_name: Optional[str] = None, auto_dataset: bool = True, dataset_index: int = 0,
                     checkpoints_dir: str = "outputs/checkpoints", proc_data_dir: str = "data/processed",
                     out_root: Optional[str] = "outputs", device="cuda") -> dict:
    """The reference's ``evaluate_model(model_type, model_name=None, auto_dataset=False)`` (`src/testing.py:26-394`) end to end on
    the HIP path: the latest ``<model_type>_*`` directory under ``checkpoints_dir`` unless ``model_name`` is given
    (``ValueError("No trained models found for type: …")`` / ``ValueError("Model not found: …")``, `:31-40`), the processed datasets
    that hold a ``test`` split (``ValueError("No processed datasets found with test data.")``, `:67`), ``best_model.pth`` before
    ``best_checkpoint.pth`` (``FileNotFoundError``, `:129`), then the loop + metrics + JSON of `evaluate_model` with results under
    ``<out_root>/<model_name>`` (`:94-96`).  The interactive dataset prompt (`:74-90`) becomes ``dataset_index`` (``auto_dataset``
    picks the first, as the reference's flag does).  Siamese pair datasets (`data_utils.SiameseDataset`) are outside the scope:
    pass pair batches to `evaluate_model` directly."""
    import os
    from pathlib import Path
    from .face_models import get_model
    ckpt_root = Path(checkpoints_dir)
    if model_name is None:
        model_dirs = list(ckpt_root.glob(f'{model_type}_*'))
        if not model_dirs:
            raise ValueError(f"No trained models found for type: {model_type}")
        model_name = sorted(model_dirs)[-1].name
    model_checkpoint_dir = ckpt_root / model_name
    if not model_checkpoint_dir.exists():
        raise ValueError(f"Model not found: {model_name}")
    processed_dirs = find_processed_datasets(proc_data_dir)
    if not processed_dirs:
        raise ValueError("No processed datasets found with test data.")
    if model_type == 'siamese':
        raise ValueError("siamese evaluation takes an iterable of (img1, img2, labels) batches: use evaluate_model")
    idx = 0 if auto_dataset else int(dataset_index)
    if not 0 <= idx < len(processed_dirs):
        raise ValueError(f"dataset_index {dataset_index} out of range (1..{len(processed_dirs)} datasets)")
    selected_data_dir, display = processed_dirs[idx]
    test_dir = selected_data_dir / "test"
    classes = sorted(d.name for d in os.scandir(test_dir) if d.is_dir())
    model = get_model(model_type, len(classes)).to(device)
    best_model_path, best_checkpoint_path = model_checkpoint_dir / 'best_model.pth', model_checkpoint_dir / 'best_checkpoint.pth'
    if best_model_path.exists():
        model.load_state_dict(torch.load(best_model_path, map_location=device, weights_only=True))
    elif best_checkpoint_path.exists():
        model.load_state_dict(torch.load(best_checkpoint_path, map_location=device, weights_only=True))
    else:
        raise FileNotFoundError(f"Neither best_model.pth nor best_checkpoint.pth found in {model_checkpoint_dir}")
    model.eval()
    out_dir = str(Path(out_root) / model_name) if out_root is not None else None
    return evaluate_model(model, model_type, str(test_dir), out_dir=out_dir, model_name=model_name, dataset_name=display, device=device)
