"""GPU: the hidden-layer head-fitting step (`frmap_head_fit_hidden_step`, csrc/head_fit.hip) and what is built on it.

THE CONTRACT (`test_kernels_against_the_twin`): over the eight shapes of `fit_hidden_cases`, at each of three steps, the kernels' h,
lab, row_src1 and z equal the host twin's bit for bit, and da, w1, b1, w2, b2 and both states equal the twin's run with `given_g` on
the device's own g.  Around it: layer 2 of the step against `frmap_head_fit_step` on clones of (h, lab, keep2, w2, b2, state 2),
kernel against kernel; determinism; `rows` as a permutation view; NaNs; guard bands at element alignment; graph replay on changed
inputs; `fit_head(hidden=...)` on a BaselineNet end to end, and `HiddenHead.embed` as the embedding of a `Gallery`."""
import os

import numpy as np
import pytest
import torch

import fit_hidden_cases as hc
import guard
from frmap_amd import head_fit as hf, matching, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
CASES = hc.cases(hc.GPU_SHAPES)
NAMES = ("w1", "b1", "w2", "b2")


def _same(a, b, what):
    a = (a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)).view(np.uint8).reshape(-1)
    b = (b.cpu().numpy() if isinstance(b, torch.Tensor) else np.ascontiguousarray(b)).view(np.uint8).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d bytes differ, first at byte %d" % (what, bad.size, int(bad[0]))


def _to(t):
    return None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(DEV)


class _Device:
    """A problem's operands on the device, from host arrays."""

    def __init__(self, p, var, fill=None):
        B, D, Hd, C = p["B"], p["D"], p["Hd"], p["C"]
        self.p, self.var = p, var
        self.x, self.labels, self.rows, self.keep1, self.keep2 = (_to(p[k]) for k in ("x", "labels", "rows", "keep1", "keep2"))
        self.w = [_to(p[k]) for k in NAMES]
        self.st = torch.zeros((hf.hidden_state_bytes(D, Hd, C, var["amsgrad"]),), dtype=torch.uint8, device=DEV)
        self.ws = torch.empty((hf.hidden_workspace_bytes(B, D, Hd, C),), dtype=torch.uint8, device=DEV)
        if fill is not None:
            self.ws.fill_(fill)
        self.scales = hc.keep_scales(var)

    def step(self, s, clear=None):
        hf.hidden_step(self.x, self.labels, *self.w, self.st, self.ws, self.rows, self.keep1, self.scales[0], self.keep2, self.scales[1],
                       **hc.step_kw(self.var, s, clear))

    def host(self):
        return [t.cpu().numpy() for t in self.w] + [self.st.cpu().numpy(), self.ws.cpu().numpy()]


def _run(p, var, steps=hc.STEPS, fill=None):
    d = _Device(p, var, fill)
    for s in range(steps):
        d.step(s)
    return d.host()


def _twin(p, var, s, w, st, ws=None, given_g=False):
    k1s, k2s = hc.keep_scales(var)
    return hf.hidden_step_host(p["x"], p["labels"], *w, st, ws, p["rows"], p["keep1"], k1s, p["keep2"], k2s, given_g=given_g,
                               **hc.step_kw(var, s))


# ---------------------------------------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[hc.case_id(c) for c in CASES])
def test_kernels_against_the_twin(case):
    """The twin runs twice a step: once on its own (h, lab, row_src1 and z: no exp or log before them) and once with `given_g` on the
    device's workspace (da, the four parameters and every state word)."""
    (B, D, Hd, C), var = case
    p = hc.problem(2000 + CASES.index(case), B, D, Hd, C, var)
    d = _Device(p, var, 0x5A)
    wt = [p[k].copy() for k in NAMES]
    stt = np.zeros(d.st.numel(), np.uint8)
    for s in range(hc.STEPS):
        what = "%s step %d" % (hc.case_id(case), s)
        own = hf.hidden_workspace_views(_twin(p, var, s, [a.copy() for a in wt], stt.copy()), B, Hd, C)
        d.step(s)
        *gw, gst, gws = d.host()
        got = hf.hidden_workspace_views(gws, B, Hd, C)
        for name in ("h", "lab", "row_src1", "z", "row_src"):
            _same(got[name], own[name], what + ": " + name)
        tws = gws.copy()
        _twin(p, var, s, wt, stt, tws, given_g=True)
        tv = hf.hidden_workspace_views(tws, B, Hd, C)
        for name in ("h", "lab", "row_src1", "da"):
            _same(got[name], tv[name], what + ": %s against the twin on the device's g" % name)
        for k, name in enumerate(NAMES):
            _same(gw[k], wt[k], what + ": " + name)
        _same(gst, stt, what + ": the states")
    n1 = hf.state_bytes(D, Hd, var["amsgrad"])
    head1, head2 = gst[:64].view(np.uint64), gst[n1: n1 + 64].view(np.uint64)
    assert head1[0] == head2[0] == hc.STEPS and head1[1] == head2[1] == B - len(p["bad"]) and not head1[2:].any()
    assert head2[2] == hc.STEPS * head2[1] and not np.array_equal(gw[0], p["w1"])


@pytest.mark.parametrize("shape", hc.GPU_SHAPES, ids=["B%d-D%d-Hd%d-C%d" % s for s in hc.GPU_SHAPES])
def test_layer_2_is_the_single_step_on_the_hidden_activations(shape):
    """Kernel against kernel: z, g, row_loss, row_src, w2, b2 and every word of the second part of the state equal
    `frmap_head_fit_step` on clones of (h, lab, keep2, w2, b2, state 2), at each of three steps."""
    B, D, Hd, C = shape
    var = hc.VARIATIONS[hc.GPU_SHAPES.index(shape) % 2]
    p = hc.problem(2100 + hc.GPU_SHAPES.index(shape), B, D, Hd, C, var)
    d = _Device(p, var)
    n1 = hf.state_bytes(D, Hd, var["amsgrad"])
    at = 8 * B * Hd + 8 * B
    for s in range(hc.STEPS):
        w2, b2, st2 = d.w[2].clone(), d.w[3].clone(), d.st[n1:].clone()
        d.step(s)
        h = d.ws[: 4 * B * Hd].clone().view(torch.float32).view(B, Hd)
        lab = d.ws[8 * B * Hd: 8 * B * Hd + 4 * B].clone().view(torch.int32)
        ws2 = torch.empty((hf.workspace_bytes(B, Hd, C),), dtype=torch.uint8, device=DEV)
        hf.step(h, lab, w2, b2, st2, ws2, None, d.keep2, d.scales[1], batch=B, **hc.step_kw(var, s))
        what = "B%d-D%d-Hd%d-C%d step %d" % (*shape, s)
        _same(ws2, d.ws[at:], what + ": z, g, row_loss and row_src")
        _same(w2, d.w[2], what + ": w2")
        _same(b2, d.w[3], what + ": b2")
        _same(st2, d.st[n1:], what + ": the second part of the state")


def test_no_masks_against_the_twin():
    """Both masks NULL: da is s itself where the gate is open."""
    B, D, Hd, C = 33, 65, 65, 33
    var = hc.NO_MASKS
    p = hc.problem(2150, B, D, Hd, C, var)
    d = _Device(p, var, 0xFF)
    wt, stt = [p[k].copy() for k in NAMES], np.zeros(d.st.numel(), np.uint8)
    for s in range(2):
        own = hf.hidden_workspace_views(_twin(p, var, s, [a.copy() for a in wt], stt.copy()), B, Hd, C)
        d.step(s)
        *gw, gst, gws = d.host()
        got = hf.hidden_workspace_views(gws, B, Hd, C)
        for name in ("h", "lab", "row_src1", "z"):
            _same(got[name], own[name], "no masks step %d: %s" % (s, name))
        tws = gws.copy()
        _twin(p, var, s, wt, stt, tws, given_g=True)
        _same(got["da"], hf.hidden_workspace_views(tws, B, Hd, C)["da"], "no masks step %d: da" % s)
        for k, name in enumerate(NAMES):
            _same(gw[k], wt[k], "no masks step %d: %s" % (s, name))
        _same(gst, stt, "no masks step %d: the states" % s)
    assert got["da"].any() and (got["da"][got["h"] <= 0] == 0).all()


def test_determinism_and_rows_as_a_view():
    B, D, Hd, C = 65, 129, 129, 129
    var = hc.VARIATIONS[0]
    p = hc.problem(2200, B, D, Hd, C, var)
    one, two = _run(p, var, fill=0xFF), _run(p, var, fill=0x5A)
    for a, b, name in zip(one, two, NAMES + ("state", "workspace")):
        _same(a, b, "the same three steps twice: " + name)
    # rows as a permutation view of the cache against the gathered copy with rows = NULL
    q = hc.problem(2201, B, D, Hd, C, var, declined=False)
    q["labels"][q["rows"][2]] = C
    q["x"][q["rows"][3], 5] = np.inf
    gathered = dict(q, x=q["x"][q["rows"]].copy(), labels=q["labels"][q["rows"]].copy(), rows=None, N=B)
    view, copy = _run(q, var), _run(gathered, var)
    for a, b, name in zip(view[:5], copy[:5], NAMES + ("state",)):
        _same(a, b, "rows as a view against the gathered copy: " + name)
    va, vb = hf.hidden_workspace_views(view[5], B, Hd, C), hf.hidden_workspace_views(copy[5], B, Hd, C)
    for name in ("h", "da", "lab", "z", "g", "row_loss"):
        _same(va[name], vb[name], "rows as a view against the gathered copy: " + name)
    assert np.array_equal(va["row_src1"][va["row_src1"] >= 0], q["rows"][va["row_src1"] >= 0]) and (va["row_src1"][[2, 3]] == -1).all()


def test_nans():
    """A NaN in w1 reaches every row of h: layer 2 declines them all and nothing changes but the workspace.  A NaN feature declines
    its own row and stays there."""
    B, D, Hd, C = 33, 65, 65, 33
    var = hc.VARIATIONS[1]
    p = hc.problem(2300, B, D, Hd, C, var, declined=False)
    d = _Device(p, var)
    d.step(0)
    before = d.host()
    d.w[0][7, 3] = float("nan")
    w1_nan = d.w[0].cpu().numpy()
    d.step(1)
    after = d.host()
    _same(after[0], w1_nan, "a NaN in w1: w1 moved")
    for k in (1, 2, 3):
        _same(after[k], before[k], "a NaN in w1: %s moved" % NAMES[k])
    n1 = hf.state_bytes(D, Hd, True)
    changed = np.flatnonzero(after[4] != before[4])
    assert set(changed.tolist()) <= set(range(8, 16)) | set(range(n1 + 8, n1 + 16)), "a NaN in w1: more than n changed in the state"
    v = hf.hidden_workspace_views(after[5], B, Hd, C)
    assert (v["row_src1"] >= 0).all() and (v["row_src"] == -1).all() and np.isnan(v["h"][:, 7]).all() and not v["da"].any()
    assert int(after[4][:8].view(np.uint64)[0]) == 1 and int(after[4][8:16].view(np.uint64)[0]) == 0
    # a NaN feature: every bit of the step equals the step whose rows entry is -1 there
    q = hc.problem(2301, B, D, Hd, C, var, declined=False)
    bad = dict(q, x=q["x"].copy())
    bad["x"][q["rows"][4], 9] = np.nan
    skipped = dict(q, rows=q["rows"].copy())
    skipped["rows"][4] = -1
    a, b = _run(bad, var, 2), _run(skipped, var, 2)
    for u, v_, name in zip(a, b, NAMES + ("state", "workspace")):
        _same(u, v_, "a NaN feature against a skipped row: " + name)
    assert not np.isnan(a[0]).any() and hf.hidden_workspace_views(a[5], B, Hd, C)["row_src1"][4] == -1


def test_guard_bands_at_element_alignment():
    """Every operand between guard bands at its element alignment (fp32 / int32 4, the masks 1, the state 8, the workspace 4: aligned
    to that and not to twice that), the state and the workspace at exactly their reported sizes, under fills 0xFF and 0x5A: the bands
    and the read-only operands stay untouched, and the results are identical under both fills and equal to the unguarded call."""
    for (B, D, Hd, C) in ((45, 70, 35, 33), (5, 2, 3, 1)):
        var = dict(hc.VARIATIONS[1], keep1=True)
        p = hc.problem(2400, B, D, Hd, C, var)
        ref = _run(p, var, 1)
        need = {"state": 8, "workspace": 4, "w1": 4, "b1": 4, "w2": 4, "b2": 4}
        k1s, k2s = hc.keep_scales(var)
        results = []
        for fill in guard.FILLS:
            g = guard.Guard(fill, device=DEV, shift=guard.min_placement(lambda dtype, kind, who: need.get(who, 1 if dtype == torch.uint8 else 4)))
            xd, ld, rd, k1d, k2d = (g.place(torch.from_numpy(p[k])) for k in ("x", "labels", "rows", "keep1", "keep2"))
            wd = [g.empty(p[k].shape, torch.float32, k) for k in NAMES]
            sd = g.empty((hf.hidden_state_bytes(D, Hd, C, True),), torch.uint8, "state")
            wsd = g.empty((hf.hidden_workspace_bytes(B, D, Hd, C),), torch.uint8, "workspace")
            assert sd.data_ptr() % 16 == 8 and wsd.data_ptr() % 8 == 4 and wd[0].data_ptr() % 8 == 4 and k1d.data_ptr() % 2 == 1 and k2d.data_ptr() % 2 == 1
            for t, k in zip(wd, NAMES):
                t.copy_(torch.from_numpy(p[k]))
            sd.zero_()
            hf.hidden_step(xd, ld, *wd, sd, wsd, rd, k1d, k1s, k2d, k2s, **hc.step_kw(var, 0))
            g.check()
            results.append([t.cpu().numpy() for t in wd] + [sd.cpu().numpy(), wsd.cpu().numpy()])
        for k, name in enumerate(NAMES + ("state", "workspace")):
            _same(results[0][k], results[1][k], "B=%d fill 0xFF against fill 0x5A: %s" % (B, name))
            _same(results[0][k], ref[k], "B=%d guarded against unguarded: %s" % (B, name))


def test_a_captured_step_replays_on_changed_inputs():
    """A captured step (one stream, no branches) replayed twice, the cache rows and both masks rewritten on the stream between the
    replays = two eager steps on those inputs: t lives in the state, and the memset of n replays."""
    B, D, Hd, C = 64, 128, 512, 36
    var = hc.VARIATIONS[0]
    p, q = hc.problem(2500, B, D, Hd, C, var), hc.problem(2501, B, D, Hd, C, var)
    q = dict(q, w1=p["w1"], b1=p["b1"], w2=p["w2"], b2=p["b2"])
    kw = hc.step_kw(var, 0, clear=False)
    eager = _Device(p, var)
    eager.step(0, clear=False)
    for name, t in (("x", eager.x), ("labels", eager.labels), ("rows", eager.rows), ("keep1", eager.keep1), ("keep2", eager.keep2)):
        t.copy_(_to(q[name]))
    eager.step(0, clear=False)
    d = _Device(p, var)
    second = {k: _to(q[k]) for k in ("x", "labels", "rows", "keep1", "keep2")}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            hf.hidden_step(d.x, d.labels, *d.w, d.st, d.ws, d.rows, d.keep1, d.scales[0], d.keep2, d.scales[1], **kw)
        for t, k in zip(d.w, NAMES):                   # (capture does not run the step; start from the same weights anyway)
            t.copy_(_to(p[k]))
        d.st.zero_()
        graph.replay()
        for name, t in (("x", d.x), ("labels", d.labels), ("rows", d.rows), ("keep1", d.keep1), ("keep2", d.keep2)):
            t.copy_(second[name])
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    for a, c, name in zip(eager.host(), d.host(), NAMES + ("state", "workspace")):
        _same(a, c, "two replays against two eager steps: " + name)
    assert int(d.st[:8].cpu().numpy().view(np.uint64)[0]) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _folder(root, classes=4, per_class=8, seed=5):
    """The synthetic image folder of `test_head_fit_gpu.py`: every class is one random base image (a 4 x 4 grid of saturated
    colours) and its samples are that image plus noise of a tenth of its contrast."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    for c in range(classes):
        os.makedirs(os.path.join(root, "class%d" % c))
        base = np.kron(rng.integers(0, 2, (4, 4, 3)) * 200.0 + 25.0, np.ones((16, 16, 1)))
        for k in range(per_class):
            img = np.clip(base + rng.normal(0, 20.0, base.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, "class%d" % c, "img%d.png" % k))
    return root


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_fit_hidden_head_end_to_end(tmp_path, calibrated_sd):
    """`fit_head(hidden=64)` for three epochs on a BaselineNet: the training loss falls and `embed` feeds a `Gallery`.  A BaselineNet's
    fc1 is Linear(128, 512), so what `load_into` takes is a fit with `hidden=512`: afterwards the model's own embedding and logits
    (the handle route) against `head.embed` / `head.logits` on `pooled_features` (the per-op conv route) by relative L2, bounded by
    2x what the same two comparisons read on the model BEFORE loading, with its own initial fc1 / fc2 - measured first."""
    import frmap_amd
    from frmap_amd import evaluate
    root = _folder(str(tmp_path / "faces"))
    model = frmap_amd.get_model("baseline", 36)
    model.load_state_dict(calibrated_sd("baseline"))
    model = model.to(DEV).eval().set_compute_dtype(torch.float16)
    x = next(evaluate._folder_batches(evaluate.image_folder(root)[0], 8, DEV))[0]
    with torch.no_grad():
        pooled = model.pooled_features(x)
        assert pooled.shape == (8, 128) and pooled.dtype == torch.float32
        emb0 = ops.linear_f32(pooled, model.fc1.weight.detach(), None, model.fc1.bias.detach(), relu=True)
        base_emb = _rel(model.get_embedding(x).float(), emb0)
        base_logits = _rel(model(x).float(), ops.linear_f32(emb0, model.fc2.weight.detach(), None, model.fc2.bias.detach()))
    print("baseline before loading: relative L2 handle route against pooled_features + linear_f32: embedding %.3g, logits %.3g" % (base_emb, base_logits))
    head, hist = hf.fit_head(model, "baseline", root, epochs=3, batch_size=8, lr=1e-2, generator=torch.Generator().manual_seed(3),
                             num_classes=36, hidden=64)
    print("fit_head hidden=64: train loss %s acc %s" % (["%.3f" % v for v in hist["train_loss"]], ["%.2f" % v for v in hist["train_acc"]]))
    assert isinstance(head, hf.HiddenHead) and (head.D, head.Hd, head.C) == (128, 64, 36) and len(hist["train_loss"]) == 3
    assert hist["train_loss"][-1] < hist["train_loss"][0]
    fig = head.epoch_figures()
    assert fig["rows"] == 32 and fig["t"] == 3 * 4
    with pytest.raises(ValueError, match="fc1"):
        head.load_into(model)
    # the embedding layer in the matcher: one enrol, one match
    feats, labels = hf.cache_features(model, "baseline", root, layer="pooled")
    assert feats.shape == (32, 128) and sorted(labels.tolist()) == [c for c in range(4) for _ in range(8)]
    emb = head.embed(feats)
    assert emb.shape == (32, 64) and float(emb.min()) >= 0.0
    first0 = int((labels == 0).nonzero()[0])
    enrolled3, probe3 = (int(i) for i in (labels == 3).nonzero()[:2, 0])
    gallery = matching.Gallery(["class0"], emb[first0: first0 + 1])
    assert gallery.append("class3", emb[enrolled3]) == 1
    name, dist, idx = matching.compare_faces(emb[probe3], gallery, 1e9)
    d0, d3 = float((emb[probe3] - emb[first0]).norm()), float((emb[probe3] - emb[enrolled3]).norm())
    assert (name, idx) == (("class3", 1) if d3 < d0 else ("class0", 0)) and abs(dist - min(d0, d3)) <= 1e-4 * max(1.0, min(d0, d3))
    z = head.logits(feats)
    want = torch.relu(feats.double() @ head.w1.double().T + head.b1.double()) @ head.w2.double().T + head.b2.double()
    assert z.shape == (32, 36) and _rel(z, want) < 1e-5
    _same(head.classifier().logits(emb), z, "classifier() on embed against logits")
    # hidden = 512: the model's own fc1 / fc2
    own, hist = hf.fit_head(model, "baseline", root, epochs=3, batch_size=8, lr=1e-2, generator=torch.Generator().manual_seed(4),
                            num_classes=36, hidden=512)
    print("fit_head hidden=512: train loss %s acc %s" % (["%.3f" % v for v in hist["train_loss"]], ["%.2f" % v for v in hist["train_acc"]]))
    assert hist["train_loss"][-1] < hist["train_loss"][0]
    before = model.get_embedding(x).float().clone()
    own.load_into(model)
    with torch.no_grad():
        got_emb, got_logits = model.get_embedding(x).float(), model(x).float()
        pooled = model.pooled_features(x)
        rel_emb, rel_logits = _rel(got_emb, own.embed(pooled)), _rel(got_logits, own.logits(pooled))
    print("baseline after load_into: relative L2 embedding %.3g (bound %.3g), logits %.3g (bound %.3g)" % (
        rel_emb, 2 * base_emb, rel_logits, 2 * base_logits))
    assert not torch.equal(before, got_emb), "load_into did not change the model's embedding"
    assert rel_emb <= 2 * base_emb and rel_logits <= 2 * base_logits
    assert torch.equal(model.fc1.weight.detach(), own.w1) and torch.equal(model.fc2.bias.detach(), own.b2)
