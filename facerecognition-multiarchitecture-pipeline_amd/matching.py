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
import weakref
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
    compare_faces' answer whenever that is a name (distances are the exact float64-summed ones, as compare_faces'
    own on every gallery size), and the list is empty when it says "Unknown".
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
    (distances are compared the same way)."""
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


def _frame_list(frames) -> list:
    """``[S, H, W, 3]`` (array or tensor) or a sequence of H×W×3 frames -> the list of frames, each checked to be H×W×3 (a
    `resize.YuvFrame` says so of the frame it converts to)."""
    fl = list(frames.unbind(0) if isinstance(frames, torch.Tensor) else frames) if getattr(frames, "ndim", 0) == 4 else list(frames)
    for f in fl:
        if len(f.shape) != 3 or f.shape[2] != 3:
            raise ValueError("expected H×W×3 uint8 BGR frames")
    return fl


def _per_stream(arg, S: int, what: str) -> list:
    if arg is None:
        return [None] * S
    if len(arg) != S:
        raise ValueError(f"{what}: {len(arg)} entries for {S} streams")
    return list(arg)


def _stream_rois(frames, boxes, probs, det_thresh, landmarks, margin):
    """The host half of the crops: per frame `frames.clip_boxes` (after `frames.margin_boxes`, and with the eye matrices, when
    asked for).  ``(rois int32 [N, 5] with the frame index first, the kept box indices per frame, matrices float64 [N, 6] or
    None)``, rows in frame order.  ``frames``: a list of H×W×3 frames; ``boxes`` / ``probs`` / ``landmarks``: one entry per frame
    (``landmarks = None``: no alignment for any frame)."""
    plain = landmarks is None and margin == 0.0
    rois, kepts, mats = [], [], []
    for s, frame in enumerate(frames):
        shape = frame.shape
        r, kept = _frames.clip_boxes(boxes[s] if plain else _frames.margin_boxes(boxes[s], margin, shape), probs[s], shape, det_thresh)
        if landmarks is not None and boxes[s] is not None:
            lm = landmarks[s]
            if lm is None or len(lm) != len(boxes[s]):
                raise ValueError(f"landmarks: {0 if lm is None else len(lm)} sets for {len(boxes[s])} boxes")
            mats.extend(_frames.rotation_matrix(*_frames.eye_rotation(lm[i])) for i in kept.tolist())
        rois.append(np.concatenate([np.full((len(kept), 1), s, np.int32), r], 1))
        kepts.append(kept)
    return np.concatenate(rois), kepts, (None if landmarks is None else np.asarray(mats, np.float64).reshape(-1, 6))


def _launch_crops(model, frames, r5, mats, size):
    """ONE crop launch over all frames: uint8 ``[N, h, w, 3]`` RGB crops on the model's device."""
    from . import resize as _resize
    dev = next(model.parameters()).device
    if mats is None:
        return _resize.crop_resize_u8(frames, r5, size, bgr=True, device=dev)
    return _resize.align_crop_resize_u8(frames, r5, mats, size, bgr=True, device=dev)


def _box_crops(model, frame, boxes, probs, size, det_thresh, landmarks=None, margin=0.0):
    """clip_boxes + one crop launch: (uint8 [n, h, w, 3] RGB crops on the model's device, kept box indices).  With ``landmarks`` /
    ``margin``: margin_boxes first, and the crops are cut out of the frame rotated about each face's eye centre."""
    shape = frame.shape
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError("expected one H×W×3 uint8 BGR frame")
    r5, kepts, mats = _stream_rois([frame], [boxes], [probs], det_thresh, None if landmarks is None else [landmarks], margin)
    return _launch_crops(model, frame, r5, mats, size), kepts[0]


def _match_records(model, u8, g, mean, std, what, normalize):
    """ONE model call on the uint8 crops and ONE match against the gallery: the int32 ``[n, 2]`` records (index, bits of the
    distance) on the device, nothing thresholded."""
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    h = model.model_handle() if what == "embedding" and hasattr(model, "model_handle") else None
    with torch.no_grad():
        if h is not None and (model.input_mean, model.input_std) == (mean, std):
            return h.embed_and_match(model._check_input(u8), g.matrix, g.prepared, float("inf"), normalize, packed=True)[3]
        emb = _probe_rows(model, u8, mean, std, what, normalize)
        return ops.match_top1(emb, g.matrix, float("inf"), packed=True, prepared=g.prepared)[3]


def _probe_rows(model, u8, mean, std, what, normalize):
    """The embed-then-match route's probes: ToTensor + Normalize, ONE model call, float32 ``[n, D]`` rows (L2-normalised for
    ``what="embedding"`` with ``normalize``)."""
    x = ops.normalize_u8(u8, mean, std)[0]
    if what == "forward":
        emb = model(x)
    else:
        emb = model.get_embedding(x)
    emb = (emb.unsqueeze(0) if emb.dim() == 1 else emb).to(torch.float32)
    if what == "embedding" and normalize:
        emb = ops.l2_normalize(emb, 1e-12)
    return emb


def _record_results(idx, dist, g, thresh) -> list:
    """`compare_faces`' triples from the host copy of match records."""
    out = []
    for i, d in zip(idx, dist):
        if i < 0:                                             # every distance NaN (see compare_faces)
            out.append(("Unknown", float('inf'), None))
        elif d <= thresh:
            out.append((g.names[i], d, i))
        else:
            out.append(("Unknown", d, None))
    return out


def embed_boxes(model, frame, boxes, probs=None, size=(160, 160), mean=(.5, .5, .5), std=(.5, .5, .5),
                det_thresh: float = _frames.DET_THRESH, landmarks=None, margin: float = 0.0):
    """The embed half of the reference's frame loop (`app.py:224-241`) for all boxes of one frame at once: `frames.clip_boxes` →
    one crop + BGR→RGB + Resize launch on the frame (`resize.crop_resize_u8`; a host frame is uploaded once) → ToTensor +
    Normalize → ONE ``model(x)`` under ``no_grad``.  ``frame``: H×W×3 uint8 BGR (cv2), host or device, or a `resize.YuvFrame`
    (an NV12 / NV21 / I420 frame: the crop launch converts the pixels it reads); ``boxes`` / ``probs``: the detector's output.  Returns ``(embeddings [n, D] on the device, kept int64 [n])``: row i is what
    ``get_embedding(frame[y1:y2, x1:x2], model)`` returns for box ``kept[i]`` (to the bit under `ops.set_batch_invariant`; to
    rounding otherwise, as for any batch); boxes below ``det_thresh`` or empty after clipping are absent.

    Aligned crops (the reference's dataset step, `src/data_prep.py:69-106, 138-150`): ``landmarks`` ``[n, >= 2, 2]`` - the
    detector's points per box, eyes first, as ``mtcnn.detect(..., landmarks=True)`` returns them - and ``margin`` (the reference's
    ``face_margin``).  Then `frames.margin_boxes` → `frames.clip_boxes` → per kept box `frames.eye_rotation` +
    `frames.rotation_matrix` → one `resize.align_crop_resize_u8` launch: each crop is cut out of the frame rotated about that
    face's eye centre until the eye line is level, resampled as PILLOW does (``Image.rotate(angle, BILINEAR, center=c)``,
    ``.crop``, ``.resize``), not as the reference's cv2 calls do.  ``margin`` alone widens the boxes of the unrotated frame."""
    u8, kept = _box_crops(model, frame, boxes, probs, size, det_thresh, landmarks, margin)
    return _embed_crops(model, u8, mean, std), kept


def _embed_crops(model, u8, mean, std):
    if u8.shape[0] == 0:
        return torch.empty((0, 0), dtype=torch.float32, device=u8.device)
    x = ops.normalize_u8(u8, mean, std)[0]
    with torch.no_grad():
        emb = model(x)
    return emb.unsqueeze(0) if emb.dim() == 1 else emb


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
    rec = _match_records(model, u8, g, mean, std, what, normalize).cpu()   # the one host copy: int32 [n, 2] = (index, bits of the distance)
    return _record_results(rec[:, 0].tolist(), rec.view(torch.float32)[:, 1].tolist(), g, thresh), kept


class StreamTracker:
    """The reference's face tracker (`app.py:183-247`; the rule is `frames.track_boxes`) for ``n_streams`` independent streams -
    cameras, or clips stepped together - with the per-stream state (previous boxes, their ids, the id counter) resident on the
    device and ONE launch per step (`ops.track_step`).  ``max_boxes``: the most detections a stream may have in one frame (up to
    256); a step with more raises ``ValueError`` before anything is uploaded: nothing is ever truncated.  ``device="cpu"`` keeps
    the state on the host and steps it with the same rule compiled for the CPU (`ops.track_step_host`): no GPU needed."""

    def __init__(self, n_streams: int, max_boxes: int = 64, device: Union[str, torch.device] = "cuda",
                 det_thresh: float = _frames.DET_THRESH, iou_thresh: float = _frames.TRACKING_THRESHOLD):
        self.n_streams, self.max_boxes = int(n_streams), int(max_boxes)
        self.device = torch.device(device)
        self.det_thresh, self.iou_thresh = float(det_thresh), float(iou_thresh)
        if self.device.type == "cpu":
            self.state = ops.track_state_host(self.n_streams, self.max_boxes)
        else:
            self.state = ops.track_state(self.n_streams, self.max_boxes, self.device)
        self.counts = np.zeros(self.n_streams, np.int32)      # of the last step
        self.device_counts = None                             # the same on the tracker's device (what `ops.track_fuse` clamps)
        self._templates = weakref.WeakSet()                   # `TrackTemplates` that follow this tracker's ids

    def pad(self, boxes, probs, frame_shapes):
        """The step's host arrays ``(boxes float32 [S, M, 4], probs float32 [S, M] or None, counts int32 [S], frame_hw int32
        [S, 2])``: views of ONE buffer (`pad.buffer`-style: the first array's ``base``), so that a single upload carries them."""
        S, M = self.n_streams, self.max_boxes
        boxes = _per_stream(boxes, S, "StreamTracker: boxes")
        probs = _per_stream(probs, S, "StreamTracker: probs")
        if len(frame_shapes) in (2, 3) and all(isinstance(v, (int, np.integer)) for v in frame_shapes):
            frame_shapes = [frame_shapes] * S                  # one (H, W[, C]) for every stream
        if len(frame_shapes) != S:
            raise ValueError(f"StreamTracker: {len(frame_shapes)} frame shapes for {S} streams")
        counts = np.array([0 if b is None else len(b) for b in boxes], np.int32)
        if counts.size and counts.max() > M:
            raise ValueError(f"StreamTracker: stream {int(counts.argmax())} has {int(counts.max())} boxes, max_boxes is {M}")
        any_probs = any(p is not None for p, c in zip(probs, counts) if c)
        buf = np.zeros(S * M * 5 + S * 3, np.float32)          # boxes | probs | counts | frame_hw, 4-byte words
        b_pad = buf[:S * M * 4].reshape(S, M, 4)
        p_pad = buf[S * M * 4:S * M * 5].reshape(S, M)
        c_pad = buf[S * M * 5:S * M * 5 + S].view(np.int32)
        hw = buf[S * M * 5 + S:].view(np.int32).reshape(S, 2)
        c_pad[:] = counts
        for s in range(S):
            hw[s] = (int(frame_shapes[s][0]), int(frame_shapes[s][1]))
            if counts[s]:
                b_pad[s, :counts[s]] = np.asarray(boxes[s], dtype=np.float32).reshape(counts[s], 4)
                if probs[s] is not None:
                    p_pad[s, :counts[s]] = np.asarray(probs[s], dtype=np.float32).reshape(counts[s])
                elif any_probs:
                    p_pad[s, :counts[s]] = np.finfo(np.float32).max   # no probabilities for this stream: every box is confident
        return b_pad, (p_pad if any_probs else None), c_pad, hw

    def step(self, boxes, probs=None, frame_shapes=None):
        """One step of every stream.  ``boxes`` / ``probs``: one entry per stream, the detector's ``[n, 4]`` boxes and ``[n]``
        probabilities (taken as float32; ``None``: no detection / every box confident); ``frame_shapes``: ``(H, W[, C])`` per stream,
        or one for all.  Pads, uploads ONCE, launches ONCE on the current stream.  Returns ``(ids int32 [S, max_boxes], rois
        int32 [S, max_boxes, 4])`` on the tracker's device (numpy arrays for ``device="cpu"``): `ops.track_step`'s outputs, nothing
        synchronised; `unpad` cuts a host copy of ``ids`` back to the streams' lengths."""
        if frame_shapes is None:
            raise ValueError("StreamTracker.step: frame_shapes is required (the crop rule depends on the frame size)")
        b_pad, p_pad, c_pad, hw = self.pad(boxes, probs, frame_shapes)
        self.counts = c_pad.copy()
        if self.device.type == "cpu":
            self.device_counts = self.counts
            return ops.track_step_host(self.state, b_pad, p_pad, c_pad, hw, self.det_thresh, self.iou_thresh)
        S, M = self.n_streams, self.max_boxes
        d = torch.from_numpy(b_pad.base).to(self.device, non_blocking=True)
        self.device_counts = d[S * M * 5:S * M * 5 + S].view(torch.int32)
        return ops.track_step(self.state, d[:S * M * 4].view(S, M, 4), None if p_pad is None else d[S * M * 4:S * M * 5].view(S, M),
                              d[S * M * 5:S * M * 5 + S].view(torch.int32), d[S * M * 5 + S:].view(torch.int32).view(S, 2),
                              self.det_thresh, self.iou_thresh)

    def unpad(self, ids) -> List[np.ndarray]:
        """Per stream, the int64 ``[n]`` ids of the last step's boxes (-1: skipped) from its padded ``ids`` (copied to the host if
        it is a device tensor, which synchronises)."""
        a = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        return [a[s, :self.counts[s]].astype(np.int64) for s in range(self.n_streams)]

    def reset(self, stream: Optional[int] = None) -> None:
        """Forget every track and restart the ids at 0, for one stream or (``None``) for all - and with them the templates of
        every `TrackTemplates` built on this tracker: the ids they are kept under start again."""
        if stream is None:
            self.state[:] = 0
        else:
            if not 0 <= stream < self.n_streams:
                raise ValueError(f"StreamTracker.reset: stream {stream} of {self.n_streams}")
            self.state[8 * stream:8 * stream + 8] = 0
        for tpl in list(self._templates):
            tpl.reset(stream)

    def next_ids(self) -> List[int]:
        """The reference's ``face_id_counter`` of every stream (one small device → host copy)."""
        meta = self.state[:8 * self.n_streams]
        meta = meta.cpu().numpy() if isinstance(meta, torch.Tensor) else meta
        return meta.view(np.int32).reshape(-1, 2)[:, 1].tolist()


class TrackTemplates:
    """The templates of a `StreamTracker`'s tracks: per track (``face_id``) the decayed sum of its embeddings and their weight,
    resident on the tracker's device and updated in ONE launch per step (`ops.track_fuse`; the rule is `frames.fuse_tracks`).  The
    state mirrors the tracker's slot for slot - after a step a stream's slots are the detections that received an id, in order -
    so a track that the tracker drops is dropped here, and an id never comes back.  ``dim``: the length of an embedding;
    ``decay``: ``0 < decay <= 1``, the weight an embedding loses per step (1: the plain mean).  ``tracker.reset`` clears the
    templates with the tracks.  On a ``device="cpu"`` tracker the same rule runs compiled for the CPU (`ops.track_fuse_host`)."""

    def __init__(self, tracker: StreamTracker, dim: int, decay: float = 1.0):
        if not isinstance(tracker, StreamTracker):
            raise ValueError("TrackTemplates: tracker must be the StreamTracker whose ids the templates follow")
        if not (0.0 < float(np.float32(decay)) <= 1.0):
            raise ValueError(f"TrackTemplates: decay = {decay} is outside (0, 1]")
        self.tracker, self.dim, self.decay = tracker, int(dim), float(decay)
        self.device = tracker.device
        if self.device.type == "cpu":
            self.state = ops.track_fuse_state_host(tracker.n_streams, tracker.max_boxes, self.dim)
        else:
            self.state = ops.track_fuse_state(tracker.n_streams, tracker.max_boxes, self.dim, self.device)
        tracker._templates.add(self)

    def step(self, ids, emb, rows):
        """Pool this step's embeddings: ``ids`` = the padded ids `StreamTracker.step` just returned, ``emb`` float32 ``[N, D]`` on
        the tracker's device, ``rows`` a HOST int32 ``[N, 2]`` = (stream, detection index) of every row.  ``rows`` is checked
        against the step's counts on the host (``ValueError`` before any state moves), uploaded, and ONE launch returns ``(fused
        [N, D], frames [N])`` (`ops.track_fuse`), nothing synchronised."""
        tr = self.tracker
        if tr.device_counts is None:
            raise ValueError("TrackTemplates.step: the tracker has not stepped yet")
        if tuple(emb.shape[1:]) != (self.dim,):
            raise ValueError(f"TrackTemplates.step: embeddings of shape {tuple(emb.shape)}, the templates hold {self.dim} values")
        if self.device.type == "cpu":
            emb = emb.detach().numpy() if isinstance(emb, torch.Tensor) else emb
            return ops.track_fuse_host(self.state, ids, tr.counts, emb, rows, self.decay)
        return ops.track_fuse(self.state, ids, tr.device_counts, emb, rows, self.decay, host_counts=tr.counts)

    def reset(self, stream: Optional[int] = None) -> None:
        """Forget the templates of one stream or (``None``) of all."""
        if stream is None:
            self.state[:] = 0
        else:
            if not 0 <= stream < self.tracker.n_streams:
                raise ValueError(f"TrackTemplates.reset: stream {stream} of {self.tracker.n_streams}")
            self.state[8 * stream:8 * stream + 8] = 0

    def unpack(self):
        """Per stream the `frames.TemplateState` (ids, weights, sums) the device holds (a device -> host copy, which synchronises)."""
        return ops.track_fuse_state_unpack(self.state, self.tracker.n_streams, self.tracker.max_boxes, self.dim)


def _stream_prepare(who, model, frames, boxes, probs, tracker, det_thresh, landmarks, margin, templates=None):
    """Everything of a stream step that can raise on the host, before any state moves: the arguments, and `clip_boxes` per
    stream.  ``(frames as a list, boxes, probs, rois int32 [N, 5], kept indices per stream, eye matrices or None)``."""
    if templates is not None:
        if tracker is None:
            raise ValueError(f"{who}: templates are kept per track id - they need the tracker they were built on")
        if not isinstance(templates, TrackTemplates) or templates.tracker is not tracker:
            raise ValueError(f"{who}: templates must be a TrackTemplates built on this tracker")
    fl = _frame_list(frames)
    S = len(fl)
    if S == 0:
        raise ValueError(f"{who}: no frames")
    boxes, probs = _per_stream(boxes, S, f"{who}: boxes"), _per_stream(probs, S, f"{who}: probs")
    landmarks = None if landmarks is None else _per_stream(landmarks, S, f"{who}: landmarks")
    if tracker is not None:
        if tracker.n_streams != S:
            raise ValueError(f"{who}: {S} frames for a tracker of {tracker.n_streams} streams")
        if det_thresh is not None and float(det_thresh) != tracker.det_thresh:
            raise ValueError(f"{who}: det_thresh = {det_thresh}, but the tracker skips boxes below {tracker.det_thresh}")
        det_thresh = tracker.det_thresh
        dev = next(model.parameters()).device
        if tracker.device.type != dev.type or tracker.device.index not in (None, dev.index):
            raise ValueError(f"{who}: the tracker lives on {tracker.device}, the model on {dev}")
        # the tracker compares float32 probabilities: `clip_boxes` gets the same float32 values, so that both keep the same boxes,
        # and a probability that is not finite (which `clip_boxes` would keep and the tracker skip) is refused here
        probs = [None if p is None else np.asarray(p, dtype=np.float32) for p in probs]
        for s, p in enumerate(probs):
            if p is not None and not np.isfinite(p).all():
                raise ValueError(f"{who}: stream {s} has a probability that is not finite")
    elif det_thresh is None:
        det_thresh = _frames.DET_THRESH
    # everything that can raise on the host - bad arguments above, `clip_boxes` on a non-finite coordinate here - raises before
    # the tracker's state moves
    return fl, boxes, probs, _stream_rois(fl, boxes, probs, det_thresh, landmarks, margin)


def _stream_step(who, model, frames, boxes, probs, tracker, size, det_thresh, landmarks, margin):
    """What `embed_streams` and `identify_streams` share: the host's clip, the tracker's launch (if any) and the one crop launch.
    ``(uint8 crops [N, h, w, 3], kept indices per stream, padded device ids or None)``."""
    fl, boxes, probs, (r5, kepts, mats) = _stream_prepare(who, model, frames, boxes, probs, tracker, det_thresh, landmarks, margin)
    ids = None
    if tracker is not None:
        ids = tracker.step(boxes, probs, [f.shape for f in fl])[0]
    whole = getattr(frames, "ndim", 0) == 4                    # a stack goes up (or is used in place) whole
    return _launch_crops(model, frames if whole else fl, r5, mats, size), kepts, ids


def _template_step(who, model, frames, boxes, probs, tracker, templates, size, det_thresh, landmarks, margin, embed):
    """A stream step with templates: the host's clip, the one crop launch, ``embed(crops)`` = the one model call, the tracker's
    launch and the one `ops.track_fuse` launch.  The crops depend on the host's clip alone, not on the tracker, so the model
    runs BEFORE the tracker here: only its output says how long an embedding is, and a length the templates do not hold is
    refused while the tracker's state has not moved.  ``(embeddings [N, D], fused [N, D], frames [N], kept indices per stream,
    padded device ids)``."""
    fl, boxes, probs, (r5, kepts, mats) = _stream_prepare(who, model, frames, boxes, probs, tracker, det_thresh, landmarks, margin,
                                                          templates)
    whole = getattr(frames, "ndim", 0) == 4
    u8 = _launch_crops(model, frames if whole else fl, r5, mats, size)
    if u8.shape[0]:
        emb = embed(u8)
        if emb.dim() != 2 or emb.shape[1] != templates.dim:
            raise ValueError(f"{who}: the model returns embeddings of shape {tuple(emb.shape)}, the templates hold {templates.dim} values")
        emb = emb.to(torch.float32)
    else:
        emb = torch.empty((0, templates.dim), dtype=torch.float32, device=u8.device)
    ids = tracker.step(boxes, probs, [f.shape for f in fl])[0]
    rows = np.concatenate([np.stack([np.full(len(k), s, np.int32), k.astype(np.int32)], 1) for s, k in enumerate(kepts)])
    fused, nframes = templates.step(ids, emb, rows)
    return emb, fused, nframes, kepts, ids


def _face_ids(tracker, ids_host, kepts, margin) -> list:
    """Per stream, the track id of every kept box.  The tracker's skip rule is `frames.clip_boxes`' on the unwidened box, so with
    ``margin == 0`` the boxes with an id are the kept boxes: checked, not assumed.  With ``margin > 0`` the crop box is widened
    and the tracker still sees the raw box: a box may be cropped yet carry -1, but only if its unwidened crop is empty."""
    out = []
    for s, kept in enumerate(kepts):
        row = ids_host[s].astype(np.int64)
        if margin == 0.0 and not np.array_equal(np.flatnonzero(row[:tracker.counts[s]] >= 0), kept):
            raise RuntimeError(f"stream {s}: the tracker gave ids to boxes {np.flatnonzero(row >= 0).tolist()}, clip_boxes kept "
                               f"{kept.tolist()} (an internal disagreement; the tracker's state has moved)")
        out.append(row[kept])
    return out


def embed_streams(model, frames, boxes, probs=None, tracker: Optional[StreamTracker] = None, size=(160, 160), mean=(.5, .5, .5),
                  std=(.5, .5, .5), det_thresh: Optional[float] = None, landmarks=None, margin: float = 0.0,
                  templates: Optional[TrackTemplates] = None):
    """`embed_boxes` for S frames - S camera streams, or S frames of a clip - in one step: per stream `frames.clip_boxes` on the
    host, then ONE tracker launch (if ``tracker``), ONE crop launch over all frames and ONE ``model(x)``.  Arguments as
    `identify_streams`.  Returns ``(embeddings [N, D] on the device, kept, offsets int64 [S + 1], ids)``: stream s owns rows
    ``offsets[s] : offsets[s + 1]``, row ``offsets[s] + i`` is box ``kept[s][i]`` of its frame - what `embed_boxes` returns for that
    frame (to the bit under `ops.set_batch_invariant`); ``ids``: the tracker's padded int32 ``[S, max_boxes]`` ids on the device
    (`StreamTracker.unpad`), or ``None``.  A frame with no kept box contributes no rows; with no rows at all no model is called.

    ``templates``: a `TrackTemplates` built on ``tracker``: after the model ONE `ops.track_fuse` launch pools every row into its
    track's template, and the return value grows to ``(embeddings, kept, offsets, ids, fused [N, D], frames [N])``: row i of
    ``fused`` is the template of row i's track after this step, ``frames[i]`` its weight (0: the row came back as it is - see
    `frames.fuse_tracks`).  Refused with ``ValueError`` before the tracker's state moves: ``templates`` without ``tracker`` or
    built on another one, and a model whose embeddings are not ``templates.dim`` long."""
    if templates is not None:
        emb, fused, nframes, kepts, ids = _template_step("embed_streams", model, frames, boxes, probs, tracker, templates, size, det_thresh,
                                                         landmarks, margin, lambda u8: _embed_crops(model, u8, mean, std))
        offsets = np.concatenate([[0], np.cumsum([len(k) for k in kepts])]).astype(np.int64)
        return emb, kepts, offsets, ids, fused, nframes
    u8, kepts, ids = _stream_step("embed_streams", model, frames, boxes, probs, tracker, size, det_thresh, landmarks, margin)
    offsets = np.concatenate([[0], np.cumsum([len(k) for k in kepts])]).astype(np.int64)
    return _embed_crops(model, u8, mean, std), kepts, offsets, ids


def identify_streams(model, frames, boxes, refs, tracker: Optional[StreamTracker] = None, thresh=REC_THRESH, probs=None,
                     size=(160, 160), mean=(.5, .5, .5), std=(.5, .5, .5), what: str = "forward", normalize: bool = False,
                     landmarks=None, margin: float = 0.0, det_thresh: Optional[float] = None,
                     templates: Optional[TrackTemplates] = None):
    """The reference's frame loop (`app.py:181-247`) between the detector and the names, as ONE step over S streams - S cameras,
    or S frames of a clip: per stream `frames.clip_boxes` (with `frames.margin_boxes` and the eye matrices as `identify_boxes`
    does them), then one tracker launch (if ``tracker``), ONE crop launch over all frames (`resize.crop_resize_u8` /
    `align_crop_resize_u8`, the ROI's frame field set to the stream), ONE model call, ONE match and ONE device → host copy that
    carries the match records and the track ids.  A model reaches its rate at hundreds of faces and a frame holds a handful: S
    calls of `identify_boxes` pay S times the launch latency for what this does once.

    ``frames``: a sequence of H×W×3 uint8 BGR frames of any sizes, or ``[S, H, W, 3]``, host or device - or a sequence of
    `resize.YuvFrame`s (NV12 / NV21 / I420, `resize.nv12_frame` ...; not mixed with packed frames): the crop launch then converts
    each pixel a filter tap reads, and the step equals the step on the converted frames bit for bit.  ``boxes`` / ``probs`` /
    ``landmarks``: one entry per stream (``None``: no detection in that frame; ``probs=None`` / ``landmarks=None``: none for any
    stream).  ``tracker``: a `StreamTracker` of S streams on the model's device, stepped once; its ``det_thresh`` is the step's
    (``det_thresh``, if given, must equal it; without a tracker it defaults to `frames.DET_THRESH`).  With a tracker the
    probabilities are taken as float32 - what a detector returns and what the tracker compares; a float64 probability within
    float32 rounding of the threshold is judged as its float32 value - and must be finite: ``ValueError`` otherwise, raised like
    every other rejection before the tracker's state has moved.  Everything else as `identify_boxes`.

    Returns, per stream, ``(results, kept, face_ids)``: ``results`` and ``kept`` exactly what `identify_boxes` returns for that
    frame (to the bit under `ops.set_batch_invariant`), ``face_ids`` int64 ``[len(kept)]``: the reference's ``face_id`` of box
    ``kept[i]`` ("Unknown #id"), or ``None`` without a tracker.  With ``margin > 0`` the tracker's skip rule still uses the
    unwidened box: a box may be cropped yet carry ``face_id = -1``, but only if its unwidened crop is empty.  A frame with no kept
    box contributes no rows; a step with no rows at all makes no model call.

    ``templates``: a `TrackTemplates` built on ``tracker`` - identify the TRACK, not only the frame.  The step then takes the
    embed-then-match route (never `frmap_model_embed_and_match`): one crop launch, ONE model call, the tracker's launch, ONE
    `ops.track_fuse` launch that pools every probe into its track's template (`frames.fuse_tracks`), `ops.l2_normalize` of the
    templates when ``normalize``, ONE `ops.match_top1` over the 2N stacked probes - the per-frame rows first, the templates behind
    them - and ONE device -> host copy.  Returns, per stream, ``(results, kept, face_ids, track_results, track_frames)``.  ``kept``
    and ``face_ids`` are those of the same call without ``templates``; ``results`` is identical bit for bit WHERE THAT CALL TAKES
    THE EMBED-THEN-MATCH ROUTE TOO (the match re-scores exactly, so a probe's record does not depend on the batch it is in).  A
    model-handle model called with ``what="embedding"`` and its own input normalisation as ``mean`` / ``std`` runs without
    templates as one `frmap_model_embed_and_match` call on the uint8 crops - another route to the same embedding, whose records
    are not promised to equal this one's to the bit.  ``track_results[i]`` is the `compare_faces` triple of the template of box ``kept[i]``'s track after this
    step, and ``track_frames[i]`` (float32) its weight - with ``decay = 1`` the number of frames pooled; 0 where the template is
    the frame's own embedding (a box without an id, or a non-finite embedding).  Refused with ``ValueError`` before the
    tracker's state moves: ``templates`` without ``tracker`` or built on another one, and a model whose output is not
    ``templates.dim`` long."""
    if what not in ("forward", "embedding"):
        raise ValueError(f"identify_streams: what must be 'forward' or 'embedding', got {what!r}")
    if templates is not None:
        return _identify_tracks(model, frames, boxes, refs, tracker, templates, thresh, probs, size, mean, std, what, normalize,
                                landmarks, margin, det_thresh)
    u8, kepts, ids = _stream_step("identify_streams", model, frames, boxes, probs, tracker, size, det_thresh, landmarks, margin)
    n = u8.shape[0]
    rec = None
    if n and refs is not None and len(refs):
        g = _as_gallery(refs, u8.device)
        rec = _match_records(model, u8, g, mean, std, what, normalize).reshape(-1)
    face_ids = [None] * len(kepts)
    if tracker is not None and n:
        # the one host copy: the int32 match records [n, 2] (if any) and the padded ids [S, max_boxes] behind them
        both = (ids.reshape(-1) if rec is None else torch.cat([rec, ids.reshape(-1)])).cpu()
        face_ids = _face_ids(tracker, both[both.numel() - ids.numel():].view(ids.shape).numpy(), kepts, margin)
        rec = None if rec is None else both[:2 * n]
    elif tracker is not None:
        face_ids = [np.zeros(0, np.int64) for _ in kepts]
    elif rec is not None:
        rec = rec.cpu()
    if rec is None:
        flat = [("Unknown", float('inf'), None)] * n
    else:
        rec = rec.view(n, 2)
        flat = _record_results(rec[:, 0].tolist(), rec.view(torch.float32)[:, 1].tolist(), g, thresh)
    out, at = [], 0
    for kept, fid in zip(kepts, face_ids):
        out.append((flat[at:at + len(kept)], kept, fid))
        at += len(kept)
    return out


def _identify_tracks(model, frames, boxes, refs, tracker, templates, thresh, probs, size, mean, std, what, normalize, landmarks,
                     margin, det_thresh):
    """`identify_streams` with templates: see there."""
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)

    def embed(u8):
        with torch.no_grad():
            return _probe_rows(model, u8, mean, std, what, normalize)
    emb, fused, nframes, kepts, ids = _template_step("identify_streams", model, frames, boxes, probs, tracker, templates, size,
                                                     det_thresh, landmarks, margin, embed)
    n = emb.shape[0]
    face_ids = [np.zeros(0, np.int64) for _ in kepts]
    flat = [("Unknown", float('inf'), None)] * (2 * n)
    host_frames = np.zeros(0, np.float32)
    if n:
        parts = []
        if refs is not None and len(refs):
            g = _as_gallery(refs, emb.device)
            if what == "embedding" and normalize:
                fused = ops.l2_normalize(fused, 1e-12)
            parts.append(ops.match_top1(torch.cat([emb, fused]), g.matrix, float("inf"), packed=True, prepared=g.prepared)[3].reshape(-1))
        # the one host copy: the int32 match records [2 n, 2] (if any), the bits of the weights [n] and the padded ids [S, max_boxes]
        both = torch.cat(parts + [nframes.view(torch.int32), ids.reshape(-1)]).cpu()
        at = both.numel() - ids.numel()
        face_ids = _face_ids(tracker, both[at:].view(ids.shape).numpy(), kepts, margin)
        host_frames = both[at - n:at].view(torch.float32).numpy()
        if parts:
            rec = both[:4 * n].view(2 * n, 2)
            flat = _record_results(rec[:, 0].tolist(), rec.view(torch.float32)[:, 1].tolist(), g, thresh)
    out, at = [], 0
    for kept, fid in zip(kepts, face_ids):
        k = len(kept)
        out.append((flat[at:at + k], kept, fid, flat[n + at:n + at + k], host_frames[at:at + k].copy()))
        at += k
    return out


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
