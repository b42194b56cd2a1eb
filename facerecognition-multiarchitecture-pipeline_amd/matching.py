"""Gallery matching with the reference's call surface, computed on the GPU.

Mirrors ``/root/reference/src/app.py``:

* ``compare_faces(emb, refs, thresh) -> (name, dist, idx|None)``  (`app.py:50-64`): Euclidean
  ``F.pairwise_distance`` (eps = 1e-6 added to the *difference*), first strict minimum, the
  ``("Unknown", dist, None)`` result above the threshold and the ``("Unknown", inf, None)``
  sentinel for ``None`` / empty input — never raises on those.
* ``load_refs()`` / ``save_refs(refs)``  (`app.py:67-123`): same pickle file layout, entries whose
  image file is missing are dropped on load; the file is read with a non-executing parser
  (``gallery_io``), not ``pickle.load``.
* ``embed_and_match(model, x, gallery, thresh)``: the batched form: for every b,
  ``ids[b], dists[b] == compare_faces(model(x[b:b+1]), refs, thresh)[2], [1]``.

The per-entry Python loop of the reference becomes one fp32 MFMA kernel
(``frmap_match_top1``) over a device-resident G×D gallery matrix.
"""
from __future__ import annotations

import contextlib
import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import frames as _frames
from . import gallery_io, ops

REC_THRESH = 1.0                       # `app.py:20`
REF_DIR = "face_references"            # `app.py:23`
REF_FILE = os.path.join(REF_DIR, "face_references.pkl")   # `app.py:24`
_save_counter = 0


class Gallery:
    """Device-resident gallery: names + one fp32 G×D matrix (row i = reference i's embedding), held in a buffer with spare
    capacity so that enrolling an identity (`app.py:428-436` appends one entry) writes ONE row - and, for galleries on the MFMA
    match path, re-packs one 64-row tile - instead of rebuilding and re-uploading everything."""

    def __init__(self, names: Sequence[str], embeddings: torch.Tensor, device: Union[str, torch.device] = "cuda"):
        emb = embeddings.detach().to(torch.float32)
        if emb.dim() == 3 and emb.shape[1] == 1:
            emb = emb[:, 0, :]
        if emb.dim() != 2 or emb.shape[0] != len(names):
            raise ValueError("Gallery: need one D-vector per name")
        self.names = list(names)
        self._buf = emb.to(device).contiguous()          # [capacity][D]; rows >= len(names) are spare
        self._pack = None
        self._label_names, self._label_of, self._label_ids = [], {}, []
        self._labels_dev = None                          # [capacity] int32, built on first use of `labels`
        self._number_labels(self.names)
        self._refresh_pack()

    def _number_labels(self, names) -> None:
        for n in names:
            lab = self._label_of.get(n)
            if lab is None:
                lab = self._label_of[n] = len(self._label_names)
                self._label_names.append(n)
            self._label_ids.append(lab)

    def _labels_current(self) -> None:
        # derived from `names`: renumber if someone replaced or edited the list behind our back
        if len(self._label_ids) != len(self.names) or (self.names and self._label_names[self._label_ids[-1]] != self.names[-1]):
            self._label_names, self._label_of, self._label_ids, self._labels_dev = [], {}, [], None
            self._number_labels(self.names)

    @property
    def label_names(self) -> List[str]:
        """The distinct names in order of first appearance: ``label_names[labels[i]] == names[i]``."""
        self._labels_current()
        return self._label_names

    @property
    def label_ids(self) -> List[int]:
        """Host copy of `labels`."""
        self._labels_current()
        return self._label_ids

    @property
    def labels(self) -> torch.Tensor:
        """int32 [G] labels on the gallery's device: each name numbered by its first appearance (the reference's `save_refs` appends
        one entry per capture, so a person can own several rows); the key of `search_batch(..., by="name")`."""
        self._labels_current()
        G = len(self.names)
        if self._labels_dev is None or self._labels_dev.shape[0] < G or self._labels_dev.device != self._buf.device:
            cap = max(self._buf.shape[0], G)
            host = torch.full((cap,), -1, dtype=torch.int32)
            host[:G] = torch.tensor(self._label_ids, dtype=torch.int32)
            self._labels_dev = host.to(self._buf.device)
        return self._labels_dev[:G]

    @property
    def matrix(self) -> torch.Tensor:
        return self._buf[: len(self.names)]

    def _wants_pack(self) -> bool:
        return ops.wants_pack(len(self.names), self._buf.shape[1])

    def _refresh_pack(self) -> None:
        # built HERE (construction / enrolment time, on the caller's stream) and guarded by an event - not lazily on whichever
        # side stream first matches against it
        if self._wants_pack() and (self._pack is None or not self._pack.matches(self.matrix)):
            with torch.cuda.device(self._buf.device):
                self._pack = ops.MatchPack(self.matrix, capacity=self._buf.shape[0])

    @property
    def prepared(self):
        """The gallery split for the MFMA match path (galleries of >= `ops.MATCH_MFMA_MIN_G` rows), else None."""
        if not self._wants_pack():
            return None
        self._refresh_pack()         # (someone wrote into `matrix` behind our back: rebuild rather than match stale rows)
        return self._pack

    def append(self, name: str, embedding: torch.Tensor) -> int:
        """Enrol one identity (`app.py:428-436`): returns its row.  One row is written on the device; the MFMA pack (if any)
        re-packs only that row's tile.  Capacity doubles when exhausted."""
        e = embedding.detach().reshape(-1).to(torch.float32)
        G, D = len(self.names), self._buf.shape[1]
        if G == 0 and D != e.numel():
            self._buf = torch.empty((16, e.numel()), dtype=torch.float32, device=self._buf.device)
            D = e.numel()
        if e.numel() != D:
            raise ValueError(f"Gallery.append: embedding has {e.numel()} values, the gallery rows have {D}")
        with (torch.cuda.device(self._buf.device) if self._buf.is_cuda else contextlib.nullcontext()):
            if G == self._buf.shape[0]:
                cap = max(2 * G, 16)
                cap = (cap + 255) // 256 * 256 if cap >= ops.MATCH_MFMA_MIN_G // 2 else cap
                grown = torch.empty((cap, D), dtype=torch.float32, device=self._buf.device)
                grown[:G] = self._buf[:G]
                self._buf, self._pack = grown, None
            self._buf[G].copy_(e.to(self._buf.device), non_blocking=True)
            self._labels_current()
            self.names.append(name)
            self._number_labels((name,))
            if self._labels_dev is not None:
                if self._labels_dev.shape[0] > G:
                    self._labels_dev[G].fill_(self._label_ids[G])    # one element; the buffer grows with the rows' capacity
                else:
                    self._labels_dev = None
            if self._wants_pack():
                if self._pack is not None and self._pack.src_ptr == self._buf.data_ptr() and self._pack.G == G:
                    self._pack.update_rows(self.matrix, G, G + 1)
                else:
                    self._pack = ops.MatchPack(self.matrix, capacity=self._buf.shape[0])
        return G

    @classmethod
    def from_refs(cls, refs: Sequence[dict], device: Union[str, torch.device] = "cuda") -> "Gallery":
        if not refs:
            return cls([], torch.zeros((0, 1)), device)
        rows = [r["embedding"].detach().reshape(-1) for r in refs]
        if len({(t.device, t.dtype) for t in rows}) == 1:
            mat = torch.stack(rows)                      # one gather on the tensors' own device, one transfer
        else:
            mat = torch.stack([t.to(torch.float32).cpu() for t in rows])
        return cls([r["name"] for r in refs], mat, device)

    def __len__(self):
        return len(self.names)


_gallery_cache: dict = {}


def _ref_tag(r) -> tuple:
    e = r.get("embedding") if isinstance(r, dict) else None
    if isinstance(e, torch.Tensor):
        return (id(e), e.data_ptr(), e._version, tuple(e.shape), r.get("name"))
    return (id(e), r.get("name") if isinstance(r, dict) else None)


def _refs_tag(refs) -> tuple:
    """Content tag of a ``refs`` list: per entry the embedding object's identity, storage address and in-place
    version counter — an in-place edit of an enrolled embedding, a replaced entry or a list that was freed and
    reallocated at the same ``id`` all change it."""
    return (len(refs),) + tuple(_ref_tag(r) for r in refs)


def _as_gallery(refs, device) -> Gallery:
    if isinstance(refs, Gallery):
        return refs
    # the demo passes the same list object every frame (`app.py:639`): keep its device matrix while the list is unchanged,
    # and when entries were only APPENDED (enrolment, `app.py:428-436`) append their rows instead of rebuilding
    key = id(refs)
    tag = _refs_tag(refs)
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    hit = _gallery_cache.get(key)
    if hit is not None and hit[1].matrix.device == dev:
        old_tag, g = hit
        if old_tag == tag:
            return g
        n_old = old_tag[0]
        if 0 < n_old < tag[0] and tag[1: 1 + n_old] == old_tag[1:] and len(g) == n_old:
            try:
                for r in refs[n_old:]:
                    g.append(r["name"], r["embedding"])
                _gallery_cache[key] = (tag, g)
                return g
            except Exception:
                pass                                     # (ragged entry: fall through to the full rebuild and its error)
    g = Gallery.from_refs(refs, dev)
    if len(_gallery_cache) > 8:
        _gallery_cache.clear()
    _gallery_cache[key] = (tag, g)
    return g


def match_batch(emb: torch.Tensor, gallery: Gallery) -> Tuple[torch.Tensor, torch.Tensor]:
    """B×D device embeddings → (int32[B] first-arg-min index, fp32[B] distance), on the device."""
    return ops.match_top1(emb.to(torch.float32), gallery.matrix, prepared=gallery.prepared)


def search_batch(emb: torch.Tensor, gallery, k: int, by: str = "entry"):
    """B×D device embeddings → the k nearest gallery entries (``by="entry"``) or people (``by="name"``: one row per name, its nearest
    enrolment) under compare_faces' exact distance: ``(idx int32[B, k], dist fp32[B, k], label int32[B, k] | None)`` on the device,
    ascending, ``(-1, inf, -1)`` past the last candidate.  ``gallery``: a `Gallery` or the reference's refs list."""
    if by not in ("entry", "name"):
        raise ValueError(f"search_batch: by must be 'entry' or 'name', got {by!r}")
    g = _as_gallery(gallery, emb.device if isinstance(emb, torch.Tensor) and emb.is_cuda else "cuda")
    e = emb.to(torch.float32)
    if e.dim() == 1:
        e = e.unsqueeze(0)
    labels = g.labels if by == "name" else None
    return ops.match_topk(e, g.matrix if len(g) else None, k, labels=labels, prepared=g.prepared if len(g) else None)


def compare_faces_topk(emb, refs, thresh, k: int, by: str = "entry"):
    """compare_faces' candidate list: at most ``k`` ``(name, dist, idx)`` with ``dist <= thresh``, ascending by (dist, idx).
    ``by="name"`` lists each person once (their nearest enrolment).  ``refs``: a refs list or a `Gallery`.  Element 0 is
    compare_faces' answer whenever that is a name (distances are the exact float64-summed ones; on galleries of <= 64 rows
    compare_faces sums in fp32 and the two can differ in the last bit), and the list is empty when it says "Unknown".
    One device -> host copy."""
    if emb is None or refs is None or len(refs) == 0:
        return []
    dev = emb.device if emb.is_cuda else torch.device("cuda")
    g = _as_gallery(refs, dev)
    e = emb.detach().reshape(1, -1).to(device=dev, dtype=torch.float32)
    idx, dist, _ = search_batch(e, g, k, by=by)
    rec = torch.stack((idx[0], dist[0].view(torch.int32))).cpu()      # the one host copy: [2, k]
    out = []
    for i, bits in zip(rec[0].tolist(), rec[1].tolist()):
        d = float(np.array([bits], dtype=np.int32).view(np.float32)[0])
        if i < 0 or not d <= thresh:
            break
        out.append((g.names[i], d, i))
    return out


def csr_by_dist(pairs: torch.Tensor, dists: torch.Tensor, counts: torch.Tensor):
    """A pair list ``(pairs [n, 2] = (i, j), dists [n], counts [B])`` in any order -> CSR ``(offsets int64 [B + 1], rows int32 [n],
    dists fp32 [n])`` with probe i's segment ``[offsets[i], offsets[i + 1])`` ordered by (dist, row): two stable sorts (by (dist, j),
    then by i).  Distances are >= 0 and never NaN, so their bit patterns order as the values do."""
    offsets = torch.zeros((counts.shape[0] + 1,), dtype=torch.int64, device=counts.device)
    torch.cumsum(counts.to(torch.int64), 0, out=offsets[1:])
    if pairs.shape[0] > 1:
        key = (dists.view(torch.int32).to(torch.int64) << 32) | pairs[:, 1].to(torch.int64)
        o1 = torch.argsort(key)
        o2 = torch.sort(pairs[o1, 0], stable=True).indices
        order = o1[o2]
        pairs, dists = pairs[order], dists[order]
    return offsets, pairs[:, 1].contiguous(), dists.contiguous()


def search_radius(emb: torch.Tensor, gallery, thresh: float):
    """B x D device embeddings -> EVERY gallery entry within ``thresh`` of each probe under compare_faces' exact distance (where
    `search_batch` lists the k nearest): CSR ``(offsets int64 [B + 1], rows int32 [n], dists fp32 [n])`` on the device, probe b's
    entries at ``[offsets[b], offsets[b + 1])`` ordered by (dist, row) - the order of `search_batch`.  ``gallery``: a `Gallery` or
    the reference's refs list.  One synchronisation (the size of the answer)."""
    g = _as_gallery(gallery, emb.device if isinstance(emb, torch.Tensor) and emb.is_cuda else "cuda")
    e = emb.to(torch.float32)
    if e.dim() == 1:
        e = e.unsqueeze(0)
    b = g.matrix if len(g) else torch.empty((0, e.shape[1]), dtype=torch.float32, device=e.device)
    pairs, dists, counts = ops.match_radius(e, thresh, b, prepared=g.prepared if len(g) else None)
    return csr_by_dist(pairs, dists, counts)


def compare_faces_all(emb, refs, thresh):
    """compare_faces' full answer: EVERY ``(name, dist, idx)`` with ``dist <= thresh`` (`app.py:50-64` names only the nearest one),
    ascending by (dist, idx); ``[]`` for a ``None`` embedding, empty refs or a bad threshold - never raises.  When non-empty its first
    element is compare_faces' answer (distances are the exact float64-summed ones; on galleries of <= 64 rows compare_faces sums in
    fp32 and the two can differ in the last bit).  ``refs``: a refs list or a `Gallery`."""
    if emb is None or refs is None or len(refs) == 0:
        return []
    try:
        dev = emb.device if emb.is_cuda else torch.device("cuda")
        g = _as_gallery(refs, dev)
        e = emb.detach().reshape(1, -1).to(device=dev, dtype=torch.float32)
        _, rows, dists = search_radius(e, g, min(float(thresh), 3.4028234663852886e38))   # (inf: every finite distance)
        rec = torch.stack((rows, dists.view(torch.int32))).cpu().numpy()      # the one host copy of the answer: [2, n]
    except (ValueError, TypeError):
        return []
    return [(g.names[int(i)], float(d), int(i)) for i, d in zip(rec[0], rec[1].view(np.float32))]


def duplicate_pairs(gallery, thresh: float, which: str = "all", labels: Optional[torch.Tensor] = None):
    """The enrolment pairs of a gallery within ``thresh`` of each other (`app.py:428-436` appends without de-duplicating):
    ``(pairs int32 [n, 2] with i < j, dists fp32 [n])`` on the device, sorted by (i, j).  ``gallery``: a `Gallery` (its own `labels`
    and prepared pack are used) or an fp32 [N, D] device tensor (then ``labels`` for ``which`` = "same" / "different": pairs of one /
    of two identities - the pairs behind a false-accept rate are ``which="different"``)."""
    if isinstance(gallery, Gallery):
        if labels is not None:
            raise ValueError("duplicate_pairs: a Gallery supplies its own labels")
        x, prep = gallery.matrix, gallery.prepared
        labels = gallery.labels if which != "all" else None
    else:
        x, prep = gallery, None
    pairs, dists, _ = ops.match_radius(x, thresh, labels_a=labels, which=which, prepared=prep)
    return pairs, dists


def components_of_pairs(n: int, pairs) -> np.ndarray:
    """Connected components of the graph on ``n`` nodes with edges ``pairs`` ([m, 2] host integers): int64 [n] cluster ids, clusters
    numbered 0, 1, ... in order of their lowest node.  Union-find, the lower root always wins, so a root IS its cluster's lowest node."""
    parent = list(range(n))

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root

    for i, j in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    roots = np.fromiter((find(v) for v in range(n)), dtype=np.int64, count=n)
    number = np.cumsum(roots == np.arange(n)) - 1          # a root's rank among the roots, in node order
    return number[roots].astype(np.int64)


def cluster_embeddings(emb: torch.Tensor, thresh: float) -> torch.Tensor:
    """Group unlabelled embeddings (a photo collection): int64 [N] cluster ids on the host = the connected components of the graph
    that joins two rows when their exact distance is <= ``thresh`` (single linkage), numbered by each cluster's lowest row.  The pair
    list comes from the device (`duplicate_pairs`); the union-find over it runs on the host."""
    x = emb.to(torch.float32)
    if x.dim() != 2:
        raise ValueError("cluster_embeddings: emb must be [N, D]")
    pairs, _ = duplicate_pairs(x, thresh)
    return torch.from_numpy(components_of_pairs(int(x.shape[0]), pairs.cpu().numpy()))


def threshold_for_far(gallery, far: float, thresholds=None) -> Tuple[Optional[float], Optional[float]]:
    """The largest threshold (of ``thresholds``, default `evaluate.default_thresholds`) at which at most a fraction ``far`` of the
    impostor pairs of ``gallery`` (a `Gallery` or a refs list; identities = `Gallery.labels`) would be accepted, and the share of
    genuine pairs accepted there: ``(threshold, tar)``, or ``(None, None)`` when no threshold qualifies.  Exact counts over every
    unordered pair of enrolments (`ops.verify_counts`, self mode).  The threshold can be passed straight to `compare_faces`
    (distances are compared the same way; on galleries of <= 64 rows compare_faces sums in fp32 and can differ in the last bit)."""
    from . import evaluate
    g = _as_gallery(gallery, "cuda")
    if len(g) < 2:
        raise ValueError("threshold_for_far: the gallery needs at least two enrolments")
    m = evaluate.verification_metrics(g.matrix, g.labels, thresholds, far_targets=(float(far),), prepared=g.prepared)
    hit = m["tar_at_far"][float(far)]
    return (None, None) if hit is None else hit


def get_embedding(face_img, model):
    """`app.py:32-48`: BGR uint8 crop → RGB → Resize((160,160)) → ToTensor → Normalize(0.5, 0.5) →
    ``model(x)`` on the model's device under ``no_grad``; ``None`` for an empty crop or on ANY
    exception (the reference swallows them, `:46-48`).  The crop is uploaded as it is; the resize (bit-exact with
    PIL's, `resize.resize_bilinear_u8`), the uint8 → normalised-float step and the model run on the GPU."""
    if face_img is None or getattr(face_img, "size", 0) == 0:
        return None
    try:
        from . import resize as _resize
        rgb = np.ascontiguousarray(np.asarray(face_img)[:, :, ::-1])
        dev = next(model.parameters()).device
        u8 = _resize.resize_bilinear_u8([rgb], (160, 160), dev)
        x = ops.normalize_u8(u8, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))[0]
        with torch.no_grad():
            return model(x)
    except Exception:
        return None


def compare_faces(emb, refs, thresh):
    """`app.py:50-64` on the GPU.  ``refs``: the reference's list of dicts (its device copy is cached and re-validated against the
    live list on every call - an O(len(refs)) walk over version counters, ~1 us per entry: fine for the demo's tens of entries) or
    a `Gallery` (no walk: what a host with thousands of identities should hold; `Gallery.append` enrols in O(1))."""
    if emb is None or refs is None or len(refs) == 0:
        return "Unknown", float('inf'), None
    dev = emb.device if emb.is_cuda else torch.device("cuda")
    g = _as_gallery(refs, dev)
    e = emb.detach().reshape(1, -1).to(device=dev, dtype=torch.float32)
    # one launch sequence, ONE device -> host copy: the int32 [1, 2] record (index, bits of the distance)
    rec = ops.match_top1(e, g.matrix, float("inf"), packed=True, prepared=g.prepared)[3].cpu()
    best_ref_idx = int(rec[0, 0])
    min_dist = float(rec.view(torch.float32)[0, 1])
    if best_ref_idx < 0:                                  # every distance NaN: the reference's loop never updates its minimum
        return "Unknown", float('inf'), None
    if min_dist <= thresh:
        return g.names[best_ref_idx], min_dist, best_ref_idx
    return "Unknown", min_dist, None


def embed_and_match(model, x: torch.Tensor, gallery, thresh: float = REC_THRESH,
                    normalize: bool = False, packed: bool = False):
    """Embed a batch and match every face.  Returns ``(ids int32[B], dists fp32[B])`` on the device,
    ``ids[b] = -1`` where the best distance exceeds ``thresh`` (compare_faces' "Unknown").
    ``normalize=True`` L2-normalises the embeddings first (for models whose embedding is not
    unit-norm: 'baseline', 'cnn', 'hybrid').  ``packed=True`` returns instead the int32 ``[B, 2]``
    record tensor ``(id, bits(dist))`` the multi-GPU all-gather ships (``dist.gather_packed``); ``packed=<tensor>``
    writes those records into the given int32 ``[B, 2]`` buffer (a slice of a larger step buffer)."""
    g = _as_gallery(gallery, x.device if isinstance(x, torch.Tensor) and x.is_cuda else "cuda")
    h = model.model_handle() if hasattr(model, "model_handle") else None
    if h is not None:
        # 'cnn' / 'arcface': forward + match as ONE call on the model handle (`frmap_model_embed_and_match`)
        _idx, dist, ids, pk, _ = h.embed_and_match(model._check_input(x), g.matrix if len(g) else None, g.prepared if len(g) else None,
                                                   thresh, normalize, packed=packed)
        return pk if (packed is not None and packed is not False) else (ids, dist)
    fmap = model.trunk_map(x) if hasattr(model, "trunk_map") and len(g) <= 64 else None
    if fmap is not None:
        # embedding == global average pool of the trunk map (ResNetTransfer): pool + normalise + match in one launch
        _idx, dist, ids, pk, _ = ops.gap_norm_match(fmap, g.matrix if len(g) else None, thresh, normalize=normalize, packed=packed)
        return pk if (packed is not None and packed is not False) else (ids, dist)
    if normalize and hasattr(model, "unit_embedding"):
        emb = model.unit_embedding(x)          # the head kernel's unit-norm output (BaselineNet)
    else:
        emb = model.get_embedding(x)
        if emb.dim() == 1:
            emb = emb.unsqueeze(0)
        if normalize:
            emb = ops.l2_normalize(emb, 1e-12)
    g = _as_gallery(gallery, emb.device)
    if packed is not None and packed is not False:
        return ops.match_top1(emb.to(torch.float32), g.matrix, thresh, packed=packed, prepared=g.prepared)[3]
    _idx, dist, ids = ops.match_top1(emb.to(torch.float32), g.matrix, thresh, prepared=g.prepared)
    return ids, dist


def _box_crops(model, frame, boxes, probs, size, det_thresh, landmarks=None, margin=0.0):
    """clip_boxes + one crop launch: (uint8 [n, h, w, 3] RGB crops on the model's device, kept box indices).  With ``landmarks`` /
    ``margin``: margin_boxes first, and the crops are cut out of the frame rotated about each face's eye centre."""
    from . import resize as _resize
    shape = frame.shape
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError("expected one H×W×3 uint8 BGR frame")
    dev = next(model.parameters()).device
    if landmarks is None and margin == 0.0:
        rois, kept = _frames.clip_boxes(boxes, probs, shape, det_thresh)
        return _resize.crop_resize_u8(frame, rois, size, bgr=True, device=dev), kept
    rois, kept = _frames.clip_boxes(_frames.margin_boxes(boxes, margin, shape), probs, shape, det_thresh)
    if landmarks is None:
        return _resize.crop_resize_u8(frame, rois, size, bgr=True, device=dev), kept
    if boxes is not None and len(landmarks) != len(boxes):
        raise ValueError(f"landmarks: {len(landmarks)} sets for {len(boxes)} boxes")
    mats = np.zeros((len(kept), 6), np.float64)
    for j, i in enumerate(kept.tolist()):
        mats[j] = _frames.rotation_matrix(*_frames.eye_rotation(landmarks[i]))
    return _resize.align_crop_resize_u8(frame, rois, mats, size, bgr=True, device=dev), kept


def embed_boxes(model, frame, boxes, probs=None, size=(160, 160), mean=(.5, .5, .5), std=(.5, .5, .5),
                det_thresh: float = _frames.DET_THRESH, landmarks=None, margin: float = 0.0):
    """The embed half of the reference's frame loop (`app.py:224-241`) for all boxes of one frame at once: `frames.clip_boxes` →
    one crop + BGR→RGB + Resize launch on the frame (`resize.crop_resize_u8`; a host frame is uploaded once) → ToTensor +
    Normalize → ONE ``model(x)`` under ``no_grad``.  ``frame``: H×W×3 uint8 BGR (cv2), host or device; ``boxes`` / ``probs``: the
    detector's output.  Returns ``(embeddings [n, D] on the device, kept int64 [n])``: row i is what
    ``get_embedding(frame[y1:y2, x1:x2], model)`` returns for box ``kept[i]`` (to the bit under `ops.set_batch_invariant`; to
    rounding otherwise, as for any batch); boxes below ``det_thresh`` or empty after clipping are absent.

    Aligned crops (the reference's dataset step, `src/data_prep.py:69-106, 138-150`): ``landmarks`` ``[n, >= 2, 2]`` - the
    detector's points per box, eyes first, as ``mtcnn.detect(..., landmarks=True)`` returns them - and ``margin`` (the reference's
    ``face_margin``).  Then `frames.margin_boxes` → `frames.clip_boxes` → per kept box `frames.eye_rotation` +
    `frames.rotation_matrix` → one `resize.align_crop_resize_u8` launch: each crop is cut out of the frame rotated about that
    face's eye centre until the eye line is level, resampled as PILLOW does (``Image.rotate(angle, BILINEAR, center=c)``,
    ``.crop``, ``.resize``), not as the reference's cv2 calls do.  ``margin`` alone widens the boxes of the unrotated frame."""
    u8, kept = _box_crops(model, frame, boxes, probs, size, det_thresh, landmarks, margin)
    if u8.shape[0] == 0:
        return torch.empty((0, 0), dtype=torch.float32, device=u8.device), kept
    x = ops.normalize_u8(u8, mean, std)[0]
    with torch.no_grad():
        emb = model(x)
    return (emb.unsqueeze(0) if emb.dim() == 1 else emb), kept


def identify_boxes(model, frame, boxes, refs, thresh=REC_THRESH, probs=None, size=(160, 160), mean=(.5, .5, .5), std=(.5, .5, .5),
                   det_thresh: float = _frames.DET_THRESH, what: str = "forward", normalize: bool = False, landmarks=None,
                   margin: float = 0.0):
    """From a frame and a detector's boxes to names: `embed_boxes`, one `ops.match_top1` against the gallery, ONE device → host
    copy.  Returns ``(results, kept)``: for box ``kept[i]``, ``results[i]`` is the ``(name, dist, ref_idx)`` triple
    ``compare_faces(get_embedding(frame[y1:y2, x1:x2], model), refs, thresh)`` returns, ``("Unknown", dist, None)`` above the
    threshold and ``("Unknown", inf, None)`` for empty ``refs`` included.  ``refs``: the reference's list or a `Gallery`.

    ``what="forward"`` matches ``model(x)``, as the reference's loop does; ``what="embedding"`` matches ``model.get_embedding(x)``
    (L2-normalised first if ``normalize``), what `embed_and_match` matches - and for a model with a model handle whose input
    normalisation (`set_input_normalization`) is ``mean`` / ``std`` the uint8 crops go straight into `frmap_model_embed_and_match`
    (`FRMAP_INPUT_U8_HWC`): no fp32 input pass.  ``landmarks`` / ``margin``: eye-aligned crops with a margin, as `embed_boxes`."""
    if what not in ("forward", "embedding"):
        raise ValueError(f"identify_boxes: what must be 'forward' or 'embedding', got {what!r}")
    u8, kept = _box_crops(model, frame, boxes, probs, size, det_thresh, landmarks, margin)
    n = u8.shape[0]
    if n == 0:
        return [], kept
    if refs is None or len(refs) == 0:
        return [("Unknown", float('inf'), None)] * n, kept
    g = _as_gallery(refs, u8.device)
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    h = model.model_handle() if what == "embedding" and hasattr(model, "model_handle") else None
    with torch.no_grad():
        if h is not None and (model.input_mean, model.input_std) == (mean, std):
            rec = h.embed_and_match(model._check_input(u8), g.matrix, g.prepared, float("inf"), normalize, packed=True)[3]
        else:
            x = ops.normalize_u8(u8, mean, std)[0]
            if what == "forward":
                emb = model(x)
            else:
                emb = model.get_embedding(x)
            emb = (emb.unsqueeze(0) if emb.dim() == 1 else emb).to(torch.float32)
            if what == "embedding" and normalize:
                emb = ops.l2_normalize(emb, 1e-12)
            rec = ops.match_top1(emb, g.matrix, float("inf"), packed=True, prepared=g.prepared)[3]
    rec = rec.cpu()                                           # the one host copy: int32 [n, 2] = (index, bits of the distance)
    out = []
    for i, d in zip(rec[:, 0].tolist(), rec.view(torch.float32)[:, 1].tolist()):
        if i < 0:                                             # every distance NaN (see compare_faces)
            out.append(("Unknown", float('inf'), None))
        elif d <= thresh:
            out.append((g.names[i], d, i))
        else:
            out.append(("Unknown", d, None))
    return out, kept


class GraphedEmbedMatch:
    """The batched embed → (normalise) → match step captured once into a HIP graph and replayed.

    One step is ~30 kernel launches of 5–150 µs; driven from Python each costs ~10 µs of host time,
    which caps how many concurrent streams can be kept fed.  Capturing the launches (hipGraph via
    ``torch.cuda.CUDAGraph`` — our kernels are plain launches on the capturing stream) removes the
    per-launch host cost, and splitting the batch over ``streams`` concurrent branches lets one
    branch's tail waves run beside another's full waves (at 256 faces the late ResNet layers have
    only 392–784 tiles for 512 workgroup slots).

    ``x`` is the static input buffer (fp32 NCHW on the device): write the next batch into
    ``pipeline.x`` (or pass it to ``__call__``, which copies it) and call; the result is the int32
    ``[B, 2]`` record tensor ``(id-or-unknown, bits(dist))`` — ``ids()`` / ``dists()`` give views.
    """

    def __init__(self, model, gallery, x: torch.Tensor, thresh: float = REC_THRESH, normalize: bool = False,
                 streams: int = 1):
        if not x.is_cuda:
            raise RuntimeError("GraphedEmbedMatch needs a device-resident input buffer (no CPU fallback)")
        self.model, self.x, self.thresh, self.normalize = model, x, float(thresh), bool(normalize)
        self.gallery = _as_gallery(gallery, x.device)
        self.streams = max(1, min(int(streams), x.shape[0]))
        self._side = [torch.cuda.Stream(device=x.device) for _ in range(self.streams - 1)]
        self._xs = list(self.x.chunk(self.streams))
        warm = torch.cuda.Stream(device=x.device)
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm), torch.no_grad():   # plans, kernel attributes, allocator pools
            for _ in range(2):
                self._run()
        torch.cuda.current_stream().wait_stream(warm)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: calls other threads make meanwhile (e.g. the NCCL watchdog polling events) must not invalidate the capture
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"), torch.no_grad():
            self.records = self._run()

    def _one(self, xs, out):
        return embed_and_match(self.model, xs, self.gallery, self.thresh, normalize=self.normalize, packed=out)

    def _run(self):
        # every micro-batch writes its records straight into its slice of one buffer (no concatenation kernel at the join)
        rec = torch.empty((self.x.shape[0], 2), dtype=torch.int32, device=self.x.device)
        if self.streams == 1:
            return self._one(self.x, rec)
        main = torch.cuda.current_stream()
        lo, slices = 0, []
        for xs in self._xs:
            slices.append(rec[lo: lo + xs.shape[0]])
            lo += xs.shape[0]
        for i, st in enumerate(self._side):
            st.wait_stream(main)
            with torch.cuda.stream(st):
                self._one(self._xs[i + 1], slices[i + 1])
        self._one(self._xs[0], slices[0])
        for st in self._side:
            main.wait_stream(st)
        return rec

    def __call__(self, x: Optional[torch.Tensor] = None) -> torch.Tensor:
        if x is not None and x.data_ptr() != self.x.data_ptr():
            self.x.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.records

    def ids(self) -> torch.Tensor:
        return self.records[:, 0]

    def dists(self) -> torch.Tensor:
        return self.records.view(torch.float32)[:, 1]


# ------------------------------------------------------------------------------------------------
# persistence (`app.py:67-123`)
# ------------------------------------------------------------------------------------------------
def _imread_bgr(path: str):
    try:
        from PIL import Image
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))[:, :, ::-1].copy()
    except Exception:
        return None


def _imwrite_bgr(path: str, img) -> bool:
    try:
        from PIL import Image
        Image.fromarray(np.asarray(img)[:, :, ::-1]).save(path)
        return True
    except Exception:
        return False


def load_refs(ref_file: Optional[str] = None) -> List[dict]:
    """`app.py:104-123`: ``[]`` if the file is missing or unreadable; entries whose image is missing
    are skipped; embeddings come back as CPU fp32 tensors."""
    ref_file = ref_file or REF_FILE
    if not os.path.exists(ref_file):
        return []
    refs = []
    try:
        for rec in gallery_io.read_gallery_file(ref_file):
            p = rec["image_path"]
            if p and os.path.exists(p):                   # as stored, relative to the working directory (`app.py:110`)
                img = _imread_bgr(p)
                if img is not None:
                    refs.append({'name': rec['name'], 'embedding': torch.tensor(rec['embedding_numpy']).cpu(),
                                 'image': img})
        return refs
    except Exception:
        return []


def save_refs(refs: Sequence[dict], ref_file: Optional[str] = None) -> bool:
    """`app.py:67-91`: one JPEG per entry (``<name>_<counter:08x>.jpg``) + the pickle list."""
    global _save_counter
    ref_file = ref_file or REF_FILE
    ref_dir = os.path.dirname(os.path.abspath(ref_file))
    try:
        os.makedirs(ref_dir, exist_ok=True)
        records = []
        for ref in refs:
            _save_counter += 1
            img_file = f"{ref['name'].replace(' ', '_')}_{_save_counter:08x}.jpg"
            img_path = os.path.join(ref_dir, img_file)
            if _imwrite_bgr(img_path, ref['image']):
                records.append({'name': ref['name'], 'embedding_numpy': ref['embedding'].detach().cpu().numpy(),
                                'image_path': img_path})
        gallery_io.write_gallery_file(ref_file, records)
        return True
    except Exception:
        return False
