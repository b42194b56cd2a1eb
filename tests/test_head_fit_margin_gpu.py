"""GPU: the margin head-fitting step (`frmap_head_fit_margin_step`, csrc/head_fit_margin.hip) and what is built on it.

THE CONTRACT (`test_kernels_against_the_twin`): over the shapes of `fit_margin_cases.GPU_SHAPES`, at each of three steps, the kernels' z
and row_src equal the host twin's bit for bit; w and the whole state equal the twin's run with `given_g` on the device's own rx, rw, g
and h; and rx, rw, cosv, g, h and the row loss are within one fp32 unit in the last place of the float64 rule evaluated on the
device's own inputs to each - the one rounding of a float64 evaluation whose own error is orders below 2^-24.  Around it: the
hand-built branch rows, determinism, `rows` as a permutation view, declined rows and NaNs, the all-declined batch, guard bands at
element alignment, graph replay on changed inputs, the synthetic fit through `MarginHead.step`, and `fit_margin_head` on an
``ArcFaceNet`` through `load_into` and `evaluate_stream`."""
import os

import numpy as np
import pytest
import torch

import fit_margin_cases as mc
import guard
from frmap_amd import head_fit as hf
from test_head_fit_margin_cpu import FIT_START, GIVEN, ROUNDED, exact_halves, within_one_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
OUT = ("w", "state", "workspace")


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
        B, D, C = p["B"], p["D"], p["C"]
        self.p, self.var = p, var
        self.x, self.labels, self.rows, self.keep, self.w = (_to(p[k]) for k in ("x", "labels", "rows", "keep", "w"))
        self.st = torch.zeros((hf.margin_state_bytes(D, C, var["amsgrad"]),), dtype=torch.uint8, device=DEV)
        self.ws = torch.empty((hf.margin_workspace_bytes(B, D, C),), dtype=torch.uint8, device=DEV)
        if fill is not None:
            self.ws.fill_(fill)

    def step(self, k, clear=None, **over):
        hf.margin_step(self.x, self.labels, self.w, self.st, self.ws, self.rows, self.keep, mc.keep_scale(self.var),
                       batch=self.p["B"], **dict(mc.step_kw(self.var, k, clear), **over))

    def host(self):
        return [t.cpu().numpy() for t in (self.w, self.st, self.ws)]


def _run(p, var, steps=mc.STEPS, fill=None, **over):
    d = _Device(p, var, fill)
    for k in range(steps):
        d.step(k, **over)
    return d.host()


def _twin(p, var, k, w, st, ws=None, given_g=False, clear=None, **over):
    return hf.margin_step_host(p["x"], p["labels"], w, st, ws, p["rows"], p["keep"], mc.keep_scale(var), given_g=given_g, batch=p["B"],
                               **dict(mc.step_kw(var, k, clear), **over))


def _check_step(p, var, kw, w_before, got, gw, gst, gws, wt, stt, what, twin_forward=True):
    """One step of the contract: `got` the device's workspace views after the step from `w_before`; `wt`, `stt` the twin's weights and
    state before it, updated in place with `given_g` on the device's workspace.  Returns the worst deviation per rounded quantity."""
    B, D, C = p["B"], p["D"], p["C"]
    if twin_forward:
        own = hf.margin_workspace_views(hf.margin_step_host(p["x"], p["labels"], wt.copy(), stt.copy(), None, p["rows"], p["keep"],
                                                            mc.keep_scale(var), batch=B, **kw), B, C)
        _same(got["z"], own["z"], what + ": z")
        _same(got["row_src"], own["row_src"], what + ": row_src")
    r64 = hf.margin_step_rule(p["x"], p["labels"], w_before.astype(np.float64), None, p["rows"], p["keep"], mc.keep_scale(var), batch=B,
                              **dict(kw, clear=False))
    mc.assert_no_knife_edge(r64, kw["easy_margin"], what)
    exact = exact_halves(p["x"], p["labels"], w_before, got, p["rows"], p["keep"], mc.keep_scale(var), dict(kw, batch=B))
    worst = {g: within_one_ulp(got[g], exact[g], what + ": " + g) for g in ROUNDED}
    tws = gws.copy()
    hf.margin_step_host(p["x"], p["labels"], wt, stt, tws, p["rows"], p["keep"], mc.keep_scale(var), given_g=True, batch=B, **kw)
    _same(tws, gws, what + ": the twin with given_g rewrote the workspace")
    _same(gw, wt, what + ": w")
    _same(gst, stt, what + ": the state")
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------------------------------------
def _contract(shape, steps=tuple(range(mc.STEPS))):
    var = mc.variation(shape)
    p = mc.problem(mc.case_seed(shape), *shape, var)
    d = _Device(p, var, 0x5A)
    wt, stt = p["w"].copy(), np.zeros(d.st.numel(), np.uint8)
    worst = dict.fromkeys(ROUNDED, 0.0)
    for k in steps:
        w_before = wt.copy()
        d.step(k)
        gw, gst, gws = d.host()
        got = hf.margin_workspace_views(gws, *shape[::2])
        for g, v in _check_step(p, var, mc.step_kw(var, k), w_before, got, gw, gst, gws, wt, stt, "%s step %d" % (mc.case_id(shape), k)).items():
            worst[g] = max(worst[g], v)
    head = gst[:64].view(np.uint64)
    assert head[0] == len(steps) and head[1] == shape[0] and head[2] == (len(steps) if steps[0] == 0 else 1) * shape[0] and head[3] <= head[2]
    return worst


@pytest.mark.parametrize("D", mc.DS)
@pytest.mark.parametrize("B", mc.BS)
def test_kernels_against_the_twin(B, D):
    """The 125 shapes, one test per (B, D) with its five C.  The twin runs twice a step: once on its own (z and row_src: nothing float64
    before them) and once with `given_g` on the device's workspace (w and every state word)."""
    worst = dict.fromkeys(ROUNDED, 0.0)
    for C in mc.CS:
        for g, v in _contract((B, D, C)).items():
            worst[g] = max(worst[g], v)
    print("kernels B %d D %d: worst fp32 units %s" % (B, D, ", ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("shape", mc.GPU_SHAPES[len(mc.CPU_SHAPES):], ids=mc.case_id)
def test_kernels_against_the_twin_at_many_workgroups(shape):
    """(1024, 512, 1000) and (64, 512, 10 000): the softmax and norm grids stride, the update runs eight chains a tile.  One step - the
    one with the easy margin and the smoothing -, since the host twin of these shapes takes seconds a step."""
    worst = _contract(shape, (1,))
    print("kernels %s: worst fp32 units %s" % (mc.case_id(shape), ", ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("easy", (False, True))
def test_every_branch_is_entered_by_its_row(easy):
    p = mc.branch_problem()
    var = mc.VARIATIONS[1]
    kw = dict(mc.BRANCH_KW, easy_margin=easy, clear=True)
    d = _Device(p, var, 0xFF)
    hf.margin_step(d.x, d.labels, d.w, d.st, d.ws, **kw)
    gw, gst, gws = d.host()
    v = hf.margin_workspace_views(gws, 6, 4)
    assert v["rx"][2] == hf.MARGIN_RMAX and v["rw"][3] == hf.MARGIN_RMAX and v["cosv"][1, 0] == F32(hf.MARGIN_HI)
    assert v["g"][1, 0] == 0.0 and v["h"][1, 0] == 0.0 and (easy or (v["g"][0, 0] == 0.0 and v["h"][0, 0] == 0.0))
    assert (v["g"][0, 0] != 0.0) == easy and not v["cosv"][2].any() and not v["cosv"][:, 3].any()
    wt, stt = p["w"].copy(), np.zeros(d.st.numel(), np.uint8)
    _check_step(p, var, kw, p["w"], v, gw, gst, gws, wt, stt, "branch rows easy=%s" % easy)
    assert gw[3].any()                                                   # the zero centre moved: rw = 1e12 times the chain, no projection


def test_one_class_one_dimension_and_the_all_declined_batch():
    var = mc.VARIATIONS[1]
    for shape in ((1, 4, 1), (5, 1, 3)):
        p = mc.problem(5, *shape, var)
        d = _Device(p, var, 0xFF)
        d.step(2)
        w, st, ws = d.host()
        v = hf.margin_workspace_views(ws, shape[0], shape[2])
        assert not v["g"].any() and not v["h"].any() and np.isfinite(v["row_loss"]).all()
        if shape[1] == 1:
            assert (np.abs(v["cosv"]) == F32(hf.MARGIN_HI)).all()
        _check_step(p, var, mc.step_kw(var, 2), p["w"], v, w, st, ws, p["w"].copy(), np.zeros(st.size, np.uint8), "B%d-D%d-C%d" % shape)
    shape = (33, 40, 65)
    p = mc.problem(2350, *shape, var)
    d = _Device(p, var)
    d.step(0)
    before = d.host()
    d.rows[::2] = -1
    d.rows[1::2] = p["N"]
    d.ws.fill_(0x5A)
    d.step(1, clear=False)
    after = d.host()
    _same(after[0], before[0], "w")
    changed = np.flatnonzero(after[1] != before[1])
    assert set(changed.tolist()) <= set(range(8, 16)) and int(after[1][8:16].view(np.uint64)[0]) == 0 and int(after[1][:8].view(np.uint64)[0]) == 1
    v = hf.margin_workspace_views(after[2], 33, 65)
    assert (v["row_src"] == -1).all() and not v["g"].any() and not v["h"].any() and not v["z"].any() and not v["rx"].any() and np.isnan(v["row_loss"]).all()
    dead = dict(p, rows=d.rows.cpu().numpy())
    tws = _twin(dead, var, 1, before[0].copy(), before[1].copy(), clear=False)
    tv = hf.margin_workspace_views(tws, 33, 65)
    within_one_ulp(v["rw"], tv["rw"].astype(np.float64), "rw of the all-declined batch")
    tv["rw"][:] = v["rw"]
    _same(after[2], tws, "the workspace of the all-declined batch against the twin's")


def test_determinism_and_rows_as_a_view():
    shape = (65, 129, 129)
    var = mc.VARIATIONS[0]
    p = mc.problem(2200, *shape, var)
    one, two = _run(p, var, fill=0xFF), _run(p, var, fill=0x5A)
    for a, b, name in zip(one, two, OUT):
        _same(a, b, "the same three steps twice: " + name)
    gathered = dict(p, x=p["x"][p["rows"]].copy(), labels=p["labels"][p["rows"]].copy(), rows=None, N=shape[0])
    copy = _run(gathered, var)
    for a, b, name in zip(one[:2], copy[:2], OUT):
        _same(a, b, "rows as a view against the gathered copy: " + name)
    va, vb = hf.margin_workspace_views(one[2], 65, 129), hf.margin_workspace_views(copy[2], 65, 129)
    for name in GIVEN:
        _same(va[name], vb[name], "rows as a view against the gathered copy: " + name)
    assert np.array_equal(va["row_src"], p["rows"]) and np.array_equal(vb["row_src"], np.arange(65))


@pytest.mark.parametrize("kind", mc.BAD_KINDS)
def test_a_declined_row_counts_for_nothing(kind):
    """The batch with the declined row inserted against the batch without it: w and the state hold the same bytes (B <= 128: one chain,
    and a +0 row is a no-op in it) and the row's workspace entries are empty."""
    shape = (33, 65, 18)
    var = mc.VARIATIONS[mc.BAD_KINDS.index(kind) % 2]
    p = mc.problem(1200, *shape, var)
    q = mc.with_bad_row(p, kind, 7)
    a, b = _run(p, var, 2), _run(q, var, 2)
    for k in range(2):
        _same(a[k], b[k], "%s: %s" % (kind, OUT[k]))
    u, v = hf.margin_workspace_views(a[2], 33, 18), hf.margin_workspace_views(b[2], 34, 18)
    others = np.arange(34) != 7
    for g in GIVEN + ("row_src",):
        _same(u[g], v[g][others] if g != "rw" else v[g], kind + ": " + g)
    assert v["row_src"][7] == -1 and not v["g"][7].any() and not v["h"][7].any() and not v["z"][7].any() and v["rx"][7] == 0 and np.isnan(v["row_loss"][7])


def test_nans():
    """A NaN feature declines its own row and stays there: every bit equals the step whose row index is -1 there.  A NaN in w reaches
    its class's column of z, every row's softmax and from there every weight (the linear step's stance: the logits are not screened)."""
    shape = (33, 65, 65)
    var = mc.VARIATIONS[1]
    p = mc.problem(2300, *shape, var)
    bad = dict(p, x=p["x"].copy())
    spoiled = int(p["rows"][4])
    bad["x"][spoiled, 9] = np.nan
    skipped = dict(p, rows=np.where(p["rows"] == spoiled, -1, p["rows"]).astype(np.int32))
    a, b = _run(bad, var, 2), _run(skipped, var, 2)
    for u, v_, name in zip(a, b, OUT):
        _same(u, v_, "a NaN feature against a skipped row: " + name)
    assert not np.isnan(a[0]).any() and hf.margin_workspace_views(a[2], 33, 65)["row_src"][4] == -1
    d = _Device(p, var)
    d.w[3, 2] = float("nan")
    d.step(0)
    v = hf.margin_workspace_views(d.ws.cpu().numpy(), 33, 65)
    assert np.isnan(v["z"][:, 3]).all() and (v["row_src"] >= 0).all() and np.isnan(v["rw"][3]) and np.isnan(v["g"]).all()


def test_guard_bands_at_element_alignment():
    """Every operand between guard bands at its element alignment (fp32 / int32 4, the mask 1, the state 8, the workspace 4: aligned to
    that and not to twice that), the state and the workspace at exactly their reported sizes, under fills 0xFF and 0x5A: the bands and
    the read-only operands stay untouched, and the results are identical under both fills and equal to the unguarded call."""
    for shape in ((23, 70, 35), (3, 2, 3), (40, 33, 130)):
        B, D, C = shape
        var = dict(mc.VARIATIONS[1], keep=True)
        p = mc.problem(2400, *shape, var)
        need = {"state": 8, "workspace": 4, "w": 4}
        results = []
        for fill in guard.FILLS:
            g = guard.Guard(fill, device=DEV, shift=guard.min_placement(lambda dtype, kind, who: need.get(who, 1 if dtype == torch.uint8 else 4)))
            xd, ld, rd, kd = (g.place(torch.from_numpy(p[k])) for k in ("x", "labels", "rows", "keep"))
            wd = g.empty(p["w"].shape, torch.float32, "w")
            sd = g.empty((hf.margin_state_bytes(D, C, True),), torch.uint8, "state")
            wsd = g.empty((hf.margin_workspace_bytes(B, D, C),), torch.uint8, "workspace")
            assert sd.data_ptr() % 16 == 8 and wsd.data_ptr() % 8 == 4 and wd.data_ptr() % 8 == 4 and kd.data_ptr() % 2 == 1 and rd.data_ptr() % 8 == 4
            wd.copy_(torch.from_numpy(p["w"]))
            sd.zero_()
            hf.margin_step(xd, ld, wd, sd, wsd, rd, kd, mc.keep_scale(var), **mc.step_kw(var, 1, True))
            g.check()
            results.append([t.cpu().numpy() for t in (wd, sd, wsd)])
        d = _Device(p, var)
        d.step(1, clear=True)
        ref = d.host()
        for k, name in enumerate(OUT):
            _same(results[0][k], results[1][k], "B=%d fill 0xFF against fill 0x5A: %s" % (B, name))
            _same(results[0][k], ref[k], "B=%d guarded against unguarded: %s" % (B, name))


def test_a_captured_step_replays_on_changed_inputs():
    """A captured step (one stream, no branches) replayed twice, the cache, the labels, the rows and the mask rewritten on the stream
    between the replays = two eager steps on those inputs: t lives in the state, and the memset of n replays."""
    shape = (64, 128, 256)
    var = mc.VARIATIONS[0]
    p, q = mc.problem(2500, *shape, var), mc.problem(2501, *shape, var)
    names = ("x", "labels", "rows", "keep")
    eager = _Device(p, var)
    eager.step(1, clear=False)
    for name in names:
        getattr(eager, name).copy_(_to(q[name]))
    eager.step(1, clear=False)
    d = _Device(p, var)
    second = {k: _to(q[k]) for k in names}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            d.step(1, clear=False)
        d.w.copy_(_to(p["w"]))                         # (capture does not run the step; start from the same weights anyway)
        d.st.zero_()
        graph.replay()
        for name in names:
            getattr(d, name).copy_(second[name])
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    for a, c, name in zip(eager.host(), d.host(), OUT):
        _same(a, c, "two replays against two eager steps: " + name)
    assert int(d.st[:8].cpu().numpy().view(np.uint64)[0]) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_synthetic_fit_through_margin_head():
    """`fit_margin_cases.FIT` through `MarginHead.step` from the CPU test's initial centres: the validation accuracy through `cosines`
    starts at 0.16796875 and ends at 0.80 or better (the float32 rule on the CPU ends at 0.82421875)."""
    f = mc.FIT
    xt, yt, xv, yv, w0, steps = mc.fit_data()
    head = hf.MarginHead(f["D"], f["classes"], DEV, amsgrad=True)
    head.weight.copy_(_to(w0))
    x, y, v = _to(xt), _to(yt), _to(xv)
    start = float((head.cosines(v).argmax(1).cpu().numpy() == yv).mean())
    for k, rows in enumerate(steps):
        m_eff, s_eff = hf.margin_schedule(k // f["steps_per_epoch"])
        head.step(x, y, _to(rows), lr=f["lr"], s=s_eff, m=m_eff, label_smoothing=0.05, decoupled=True, weight_decay=1e-4)
    fig = head.epoch_figures()
    cos = head.cosines(v).cpu().numpy()
    end = float((cos.argmax(1) == yv).mean())
    print("synthetic fit, MarginHead.step: validation accuracy %.8f -> %.8f, train loss %.4f accuracy %.3f" % (start, end, fig["loss"], fig["accuracy"]))
    assert fig["t"] == f["steps"] and fig["rows"] == f["steps"] * f["batch"]
    assert start == FIT_START and end >= 0.80, (start, end)
    want = mc.unit(xv) @ mc.unit(head.weight.cpu().numpy()).T
    assert np.abs(cos - want).max() <= 1e-5 and torch.equal(head.logits(v, 1.0), head.cosines(v))


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


def test_fit_margin_head_end_to_end(tmp_path, calibrated_sd):
    """`fit_margin_head` for thirty epochs (through the warm-up and twenty epochs beyond it) on an ArcFaceNet: a [36, 512] head over its
    normalised embeddings, four of the classes present.  After `load_into` the model's own classification path - `evaluate_stream`,
    which scores `cosine_logits(emb, arcface.weight)` - has exactly the accuracy of the head's cosines on the cache, at least the 0.9
    that `test_head_fit_gpu.py` asks of the softmax head on the same folder, and `arcface_validate` the head's arg-max."""
    import frmap_amd
    from frmap_amd import evaluate
    root = _folder(str(tmp_path / "faces"))
    model = frmap_amd.get_model("arcface", 36)
    model.load_state_dict(calibrated_sd("arcface"))
    model = model.to(DEV).eval().set_compute_dtype(torch.float16)
    head, hist = hf.fit_margin_head(model, root, val_data=root, epochs=30, batch_size=8, lr=1e-2, num_classes=36,
                                    generator=torch.Generator().manual_seed(3))
    print("fit_margin_head: train loss %s acc %s val acc %s" % (["%.3f" % v for v in hist["train_loss"]], ["%.2f" % v for v in hist["train_acc"]],
                                                              ["%.2f" % m["accuracy"] for m in hist["val"]]))
    assert isinstance(head, hf.MarginHead) and (head.D, head.C) == (512, 36) and len(hist["train_loss"]) == 30 and len(hist["val"]) == 30
    fig = head.epoch_figures()
    assert fig["rows"] == 32 and fig["t"] == 30 * 4
    assert hist["val"][-1]["rows"] == 32 and hist["val"][-1]["accuracy"] >= hist["val"][0]["accuracy"]
    feats, labels = hf.cache_embeddings(model, root)
    assert feats.shape == (32, 512) and float((feats.norm(dim=1) - 1).abs().max()) < 1e-3
    own = float((head.cosines(feats).argmax(1) == labels).float().mean())
    before = evaluate.evaluate_stream(model, "arcface", root, device=DEV)
    head.load_into(model)
    assert torch.equal(model.arcface.weight.detach(), head.weight)
    after = evaluate.evaluate_stream(model, "arcface", root, device=DEV)
    print("arcface after load_into: accuracy %.3f -> %.3f (the head's own %.3f)" % (before["accuracy"], after["accuracy"], own))
    assert after["rows"] == 32 and after["accuracy"] == own == hist["val"][-1]["accuracy"] and own >= 0.9
    x = next(evaluate._folder_batches(evaluate.image_folder(root)[0], 8, DEV))[0]
    logits, arg = evaluate.arcface_validate(model, x)
    assert arg.tolist() == head.cosines(model.get_embedding(x).float()).argmax(1).tolist()


def test_fit_margin_head_draws_in_the_documented_order():
    """`fit_margin_head` against the same fit replayed by hand, N = 20, D = 8, C = 3, batches of 8 (the last one has 4 rows), 2 epochs,
    dropout 0.25: the device generator's seed from the CPU generator FIRST, then the head from it (the reverse of `fit_head`); per epoch
    `margin_schedule(epoch)` and one `randperm`; per batch one mask `rand`; `head.step`.  The centres, the whole state and the history
    are equal."""
    from test_head_fit_gpu import _FlatTrunk
    rng = np.random.default_rng(9)
    data = [(torch.from_numpy(rng.standard_normal((n, 2, 2, 2)).astype(F32)), torch.from_numpy(rng.integers(0, 3, n))) for n in (12, 8)]
    data[0][1][:3] = torch.tensor([0, 1, 2])
    trunk, kw = _FlatTrunk(), dict(lr=1e-2, weight_decay=1e-4, label_smoothing=0.05, decoupled=True)
    epochs, batch, dropout, s, m = 2, 8, 0.25, 32.0, 0.5
    got, hist = hf.fit_margin_head(trunk, data, epochs=epochs, batch_size=batch, dropout=dropout, s=s, m=m, amsgrad=True, device=DEV,
                                   generator=torch.Generator().manual_seed(21), **kw)
    feats, labels = hf.cache_embeddings(trunk, data, device=DEV)
    N, D = feats.shape
    assert (N, D, int(labels.max()) + 1) == (20, 8, 3)
    gen = torch.Generator().manual_seed(21)
    dev_gen = torch.Generator(device=DEV)
    dev_gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=gen).item()))
    head = hf.MarginHead(D, 3, DEV, amsgrad=True, generator=gen)
    want = {"train_loss": [], "train_acc": [], "val": []}
    sizes = []
    for epoch in range(epochs):
        m_eff, s_eff = hf.margin_schedule(epoch, s, m)
        perm = torch.randperm(N, device=DEV, generator=dev_gen).to(torch.int32)
        head.new_epoch()
        for lo in range(0, N, batch):
            rows = perm[lo: lo + batch]
            sizes.append(int(rows.shape[0]))
            keep = (torch.rand((rows.shape[0], D), device=DEV, generator=dev_gen) >= dropout).to(torch.uint8)
            head.step(feats, labels, rows, keep, s=s_eff, m=m_eff, dropout=dropout, **kw)
        fig = head.epoch_figures()
        want["train_loss"].append(fig["loss"])
        want["train_acc"].append(fig["accuracy"])
    assert sizes == [8, 8, 4] * epochs
    assert type(got) is type(head)
    for name in ("weight", "state"):
        assert torch.equal(getattr(got, name), getattr(head, name)), name
    assert hist == want and len(hist["train_loss"]) == epochs and got.epoch_figures()["t"] == 3 * epochs
