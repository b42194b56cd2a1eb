"""GPU: the pair head-fitting step (`frmap_head_fit_pair_step`, csrc/head_fit_pair.hip) and what is built on it.

THE CONTRACT (`test_kernels_against_the_twin`): over the shapes of `fit_pair_cases.GPU_SHAPES`, at each of three steps, the kernels' a
and row_src equal the host twin's bit for bit; w, b and the whole state equal the twin's run with `given_g` on the device's own ga;
and ga, pair_loss and dist are within one fp32 unit in the last place of the float64 rule's value on the device's a - the one
rounding of a float64 evaluation whose own error is orders below 2^-24.  Around it: the forward against the hidden-layer step's h,
kernel against kernel; determinism; the pair lists as a permutation view; bad pairs and NaNs; the all-declined batch; guard bands at
element alignment; graph replay on changed inputs; the synthetic fit through `PairHead.step`; `PairHead.embed` in a `Gallery`;
`fit_pair_head` on a SiameseNet end to end."""
import os

import numpy as np
import pytest
import torch

import fit_pair_cases as pc
import guard
from frmap_amd import head_fit as hf, matching

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
CASES = pc.cases(pc.GPU_SHAPES)
OUT = ("w", "b", "state", "workspace")


def _same(a, b, what):
    a = (a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)).view(np.uint8).reshape(-1)
    b = (b.cpu().numpy() if isinstance(b, torch.Tensor) else np.ascontiguousarray(b)).view(np.uint8).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d bytes differ, first at byte %d" % (what, bad.size, int(bad[0]))


def within_one_ulp(got32, exact64, what):
    """|got - exact| <= one fp32 unit in the last place of the exact value; NaNs in the same places.  Returns the worst, in ulps."""
    got, exact = np.asarray(got32, F32).astype(np.float64).reshape(-1), np.asarray(exact64, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(exact)), what + ": NaNs in different places"
    ok = ~np.isnan(exact)
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.abs(exact[ok]).astype(F32)).astype(np.float64)
    worst = float((np.abs(got[ok] - exact[ok]) / ulp).max()) if ok.any() else 0.0
    assert worst <= 1.0, "%s: %.3f fp32 units in the last place from the float64 value" % (what, worst)
    return worst


def _to(t):
    return None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(DEV)


class _Device:
    """A problem's operands on the device, from host arrays."""

    def __init__(self, p, var, fill=None):
        P, D, E = p["P"], p["D"], p["E"]
        self.p, self.var = p, var
        self.x, self.left, self.right, self.differ, self.keep = (_to(p[k]) for k in ("x", "left", "right", "differ", "keep"))
        self.w, self.b = _to(p["w"]), _to(p["b"])
        self.st = torch.zeros((hf.pair_state_bytes(D, E, var["amsgrad"]),), dtype=torch.uint8, device=DEV)
        self.ws = torch.empty((hf.pair_workspace_bytes(P, D, E),), dtype=torch.uint8, device=DEV)
        if fill is not None:
            self.ws.fill_(fill)

    def step(self, s, clear=None):
        hf.pair_step(self.x, self.left, self.right, self.differ, self.w, self.b, self.st, self.ws, self.keep, pc.keep_scale(self.var),
                     **pc.step_kw(self.var, s, clear))

    def host(self):
        return [t.cpu().numpy() for t in (self.w, self.b, self.st, self.ws)]


def _run(p, var, steps=pc.STEPS, fill=None):
    d = _Device(p, var, fill)
    for s in range(steps):
        d.step(s)
    return d.host()


def _twin(p, var, s, w, b, st, ws=None, given_g=False, clear=None):
    return hf.pair_step_host(p["x"], p["left"], p["right"], p["differ"], w, b, st, ws, p["keep"], pc.keep_scale(var), given_g=given_g,
                             **pc.step_kw(var, s, clear))


# ---------------------------------------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[pc.case_id(c) for c in CASES])
def test_kernels_against_the_twin(case):
    """The twin runs twice a step: once on its own (a and row_src: nothing float64 before them) and once with `given_g` on the device's
    workspace (w, b and every state word).  Measured on an MI355X: the worst ga / pair_loss / dist over all cases is 0.500 ulp - the
    device's float64 value rounds to the float64 rule's fp32 neighbour or to that value itself."""
    (P, D, E), var = case
    p = pc.problem(pc.case_seed(case), P, D, E, var)
    d = _Device(p, var, 0x5A)
    wt, bt, stt = p["w"].copy(), p["b"].copy(), np.zeros(d.st.numel(), np.uint8)
    worst = 0.0
    for s in range(pc.STEPS):
        what = "%s step %d" % (pc.case_id(case), s)
        own = hf.pair_workspace_views(_twin(p, var, s, wt.copy(), bt.copy(), stt.copy()), P, E)
        d.step(s)
        gw, gb, gst, gws = d.host()
        got = hf.pair_workspace_views(gws, P, E)
        _same(got["a"], own["a"], what + ": a")
        _same(got["row_src"], own["row_src"], what + ": row_src")
        n = int(gst[8:16].view(np.uint64)[0])
        loss64, d64, gl, gr = hf.pair_loss_rule(got["a"][:P], got["a"][P:], p["differ"], n, *pc.LOSS_F32)
        pc.assert_no_knife_edge(d64, what)
        worst = max(worst, within_one_ulp(got["ga"], np.concatenate([gl, gr]), what + ": ga"),
                    within_one_ulp(got["pair_loss"], loss64, what + ": pair_loss"), within_one_ulp(got["dist"], d64, what + ": dist"))
        tws = gws.copy()
        _twin(p, var, s, wt, bt, stt, tws, given_g=True)
        _same(tws, gws, what + ": the twin with given_g rewrote the workspace")
        _same(gw, wt, what + ": w")
        _same(gb, bt, what + ": b")
        _same(gst, stt, what + ": the state")
    head = gst[:64].view(np.uint64)
    assert head[0] == pc.STEPS and head[1] == P and head[2] == pc.STEPS * P and head[3] <= head[2] and not np.array_equal(gw, p["w"])
    print("%s: worst ga / pair_loss / dist %.3f ulp" % (pc.case_id(case), worst))


def test_forward_is_the_hidden_steps_first_layer_on_non_negative_operands():
    """Kernel against kernel: with x, w and b >= 0 the ReLU is the identity, and a [2P, E] holds the bits of the h that
    `frmap_head_fit_hidden_step` forms from rows = left ++ right with every label valid - the same tile walk, another epilogue."""
    for (P, D, E), var in (((33, 129, 65), pc.VARIATIONS[0]), ((16, 64, 32), pc.VARIATIONS[1])):
        p = pc.problem(2100, P, D, E, var)
        p.update(x=np.abs(p["x"]), w=np.abs(p["w"]), b=np.abs(p["b"]))
        d = _Device(p, var)
        d.step(0)
        a = hf.pair_workspace_views(d.ws.cpu().numpy(), P, E)["a"]
        rows = torch.cat([d.left, d.right])
        w2, b2 = torch.zeros((2, E), device=DEV), torch.zeros((2,), device=DEV)
        st = torch.zeros((hf.hidden_state_bytes(D, E, 2),), dtype=torch.uint8, device=DEV)
        ws = torch.empty((hf.hidden_workspace_bytes(2 * P, D, E, 2),), dtype=torch.uint8, device=DEV)
        hf.hidden_step(d.x, torch.zeros((p["N"],), dtype=torch.int32, device=DEV), _to(p["w"]), _to(p["b"]), w2, b2, st, ws, rows, d.keep,
                       pc.keep_scale(var), lr=1e-3)
        h = hf.hidden_workspace_views(ws.cpu().numpy(), 2 * P, E, 2)["h"]
        assert (a > 0).all()
        _same(a, h, "P%d-D%d-E%d: a against the hidden step's h" % (P, D, E))


def test_determinism_and_pairs_as_a_view():
    P, D, E = 65, 129, 129
    var = pc.VARIATIONS[0]
    p = pc.problem(2200, P, D, E, var)
    one, two = _run(p, var, fill=0xFF), _run(p, var, fill=0x5A)
    for a, b, name in zip(one, two, OUT):
        _same(a, b, "the same three steps twice: " + name)
    # left / right as a permutation view of the cache against the gathered copy with left = 0 .. P-1, right = P .. 2P-1
    idx = np.concatenate([p["left"], p["right"]])
    gathered = dict(p, x=p["x"][idx].copy(), left=np.arange(P, dtype=np.int32), right=np.arange(P, 2 * P, dtype=np.int32), N=2 * P)
    copy = _run(gathered, var)
    for a, b, name in zip(one[:3], copy[:3], OUT):
        _same(a, b, "pairs as a view against the gathered copy: " + name)
    va, vb = hf.pair_workspace_views(one[3], P, E), hf.pair_workspace_views(copy[3], P, E)
    for name in ("a", "ga", "pair_loss", "dist"):
        _same(va[name], vb[name], "pairs as a view against the gathered copy: " + name)
    assert np.array_equal(va["row_src"], idx) and np.array_equal(vb["row_src"], np.arange(2 * P))


@pytest.mark.parametrize("kind", pc.BAD_KINDS)
def test_a_bad_pair_counts_for_nothing(kind):
    """The batch with the bad pair inserted against the batch without it: w, b and the state hold the same bytes (2P <= 128: one chain,
    and a +0 row is a no-op in it) and the pair's workspace rows are empty."""
    P, D, E = 17, 65, 33
    var = pc.VARIATIONS[pc.BAD_KINDS.index(kind) % 2]
    p = pc.problem(1200, P, D, E, var)
    q = pc.with_bad_pair(p, kind, 5)
    a, b = _run(p, var, 2), _run(q, var, 2)
    for k in range(3):
        _same(a[k], b[k], "%s: %s" % (kind, OUT[k]))
    v, u = hf.pair_workspace_views(b[3], P + 1, E), hf.pair_workspace_views(a[3], P, E)
    assert v["row_src"][5] == -1 and v["row_src"][P + 1 + 5] == -1 and (v["row_src"][[4, 6]] >= 0).all()
    assert not v["ga"][5].any() and not v["ga"][P + 1 + 5].any() and np.isnan(v["pair_loss"][5]) and np.isnan(v["dist"][5])
    good = np.delete(np.arange(P + 1), 5)
    _same(v["ga"][good], u["ga"][:P], kind + ": ga of the left rows of the other pairs")
    _same(v["dist"][good], u["dist"], kind + ": dist of the other pairs")


def test_nans():
    """A NaN in w reaches every row of a and from there every weight (the linear step's stance: the logits are not screened).  A NaN
    feature declines its own pair and stays there: every bit equals the step whose left index is -1 there."""
    P, D, E = 33, 65, 65
    var = pc.VARIATIONS[1]
    p = pc.problem(2300, P, D, E, var)
    bad = dict(p, x=p["x"].copy())
    spoiled = int(p["left"][4])
    bad["x"][spoiled, 9] = np.nan
    skipped = dict(p, left=np.where((p["left"] == spoiled), -1, p["left"]).astype(np.int32),
                   right=np.where((p["right"] == spoiled), -1, p["right"]).astype(np.int32))
    a, b = _run(bad, var, 2), _run(skipped, var, 2)
    for u, v_, name in zip(a, b, OUT):
        _same(u, v_, "a NaN feature against skipped pairs: " + name)
    assert not np.isnan(a[0]).any() and hf.pair_workspace_views(a[3], P, E)["row_src"][4] == -1
    d = _Device(p, var)
    d.w[3, 2] = float("nan")
    d.step(0)
    v = hf.pair_workspace_views(d.ws.cpu().numpy(), P, E)
    assert np.isnan(v["a"][:, 3]).all() and (v["row_src"] >= 0).all() and np.isnan(v["ga"]).all() and np.isnan(d.w.cpu().numpy()).all()


def test_an_all_declined_batch_changes_nothing_but_the_workspace():
    P, D, E = 33, 40, 65
    var = pc.VARIATIONS[1]
    p = pc.problem(2350, P, D, E, var)
    d = _Device(p, var)
    d.step(0)
    before = d.host()
    d.differ.fill_(2)
    d.left[::2] = -1
    d.ws.fill_(0x5A)
    d.step(1, clear=False)
    after = d.host()
    _same(after[0], before[0], "w")
    _same(after[1], before[1], "b")
    changed = np.flatnonzero(after[2] != before[2])
    assert set(changed.tolist()) <= set(range(8, 16)) and int(after[2][8:16].view(np.uint64)[0]) == 0 and int(after[2][:8].view(np.uint64)[0]) == 1
    v = hf.pair_workspace_views(after[3], P, E)
    assert (v["row_src"] == -1).all() and not v["ga"].any() and np.isnan(v["pair_loss"]).all() and np.isnan(v["dist"]).all()
    assert v["a"][1].any() and not v["a"][0].any()
    dead = dict(p, differ=np.full(P, 2, np.int32), left=d.left.cpu().numpy())
    _same(after[3], _twin(dead, var, 1, before[0].copy(), before[1].copy(), before[2].copy(), clear=False),
          "the workspace of the all-declined batch against the twin's")


def test_guard_bands_at_element_alignment():
    """Every operand between guard bands at its element alignment (fp32 / int32 4, the mask 1, the state 8, the workspace 4: aligned to
    that and not to twice that), the state and the workspace at exactly their reported sizes, under fills 0xFF and 0x5A: the bands and
    the read-only operands stay untouched, and the results are identical under both fills and equal to the unguarded call."""
    for (P, D, E) in ((23, 70, 35), (3, 2, 3), (5, 9, pc.REG_E + 1)):
        var = dict(pc.VARIATIONS[1], keep=True)
        p = pc.problem(2400, P, D, E, var)
        ref = _run(p, var, 1)
        need = {"state": 8, "workspace": 4, "w": 4, "b": 4}
        results = []
        for fill in guard.FILLS:
            g = guard.Guard(fill, device=DEV, shift=guard.min_placement(lambda dtype, kind, who: need.get(who, 1 if dtype == torch.uint8 else 4)))
            xd, ld, rd, dd, kd = (g.place(torch.from_numpy(p[k])) for k in ("x", "left", "right", "differ", "keep"))
            wd, bd = g.empty(p["w"].shape, torch.float32, "w"), g.empty(p["b"].shape, torch.float32, "b")
            sd = g.empty((hf.pair_state_bytes(D, E, True),), torch.uint8, "state")
            wsd = g.empty((hf.pair_workspace_bytes(P, D, E),), torch.uint8, "workspace")
            assert sd.data_ptr() % 16 == 8 and wsd.data_ptr() % 8 == 4 and wd.data_ptr() % 8 == 4 and kd.data_ptr() % 2 == 1 and ld.data_ptr() % 8 == 4
            wd.copy_(torch.from_numpy(p["w"]))
            bd.copy_(torch.from_numpy(p["b"]))
            sd.zero_()
            hf.pair_step(xd, ld, rd, dd, wd, bd, sd, wsd, kd, pc.keep_scale(var), **pc.step_kw(var, 0))
            g.check()
            results.append([t.cpu().numpy() for t in (wd, bd, sd, wsd)])
        for k, name in enumerate(OUT):
            _same(results[0][k], results[1][k], "P=%d fill 0xFF against fill 0x5A: %s" % (P, name))
            _same(results[0][k], ref[k], "P=%d guarded against unguarded: %s" % (P, name))


def test_a_captured_step_replays_on_changed_inputs():
    """A captured step (one stream, no branches) replayed twice, the cache, the pair lists and the mask rewritten on the stream between
    the replays = two eager steps on those inputs: t lives in the state, and the memset of n replays."""
    P, D, E = 64, 128, 256
    var = pc.VARIATIONS[0]
    p, q = pc.problem(2500, P, D, E, var), pc.problem(2501, P, D, E, var)
    names = ("x", "left", "right", "differ", "keep")
    eager = _Device(p, var)
    eager.step(0, clear=False)
    for name in names:
        getattr(eager, name).copy_(_to(q[name]))
    eager.step(0, clear=False)
    d = _Device(p, var)
    second = {k: _to(q[k]) for k in names}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            d.step(0, clear=False)
        d.w.copy_(_to(p["w"]))                         # (capture does not run the step; start from the same weights anyway)
        d.b.copy_(_to(p["b"]))
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
def test_the_synthetic_fit_through_pair_head():
    """`fit_pair_cases.FIT` through `PairHead.step`: the validation EER of `embed` is at most HALF the raw features' EER (the CPU file
    shows that the rule alone reaches a third: that is the margin).  Measured on an MI355X: raw 0.4745, fitted 0.0935."""
    f = pc.FIT
    xt, yt, xv, yv, steps = pc.fit_data()
    head = hf.PairHead(f["D"], f["E"], DEV, generator=torch.Generator().manual_seed(f["seed"]))
    x = _to(xt)
    for left, right, differ in steps:
        head.step(x, _to(left), _to(right), _to(differ), lr=f["lr"])
    fig = head.epoch_figures()
    emb = head.embed(_to(xv)).cpu().numpy()
    raw, fitted = pc.eer(xv, yv), pc.eer(emb, yv)
    print("synthetic fit, PairHead.step: raw EER %.4f, fitted EER %.4f, train loss %.4f accuracy %.3f" % (raw, fitted, fig["loss"], fig["accuracy"]))
    assert fig["t"] == f["steps"] and fig["rows"] == f["steps"] * f["pairs"] and 0.5 < fig["accuracy"] <= 1.0
    assert np.abs(np.sqrt((emb.astype(np.float64) ** 2).sum(axis=1)) - 1).max() < 1e-5
    assert fitted <= raw / 2, (raw, fitted)
    # the embedding layer in the matcher: one enrol, one match
    e = head.embed(_to(xv))
    first0, (en3, pr3) = int(np.flatnonzero(yv == 0)[0]), (int(i) for i in np.flatnonzero(yv == 3)[:2])
    gallery = matching.Gallery(["class0"], e[first0: first0 + 1])
    assert gallery.append("class3", e[en3]) == 1
    name, dist, idx = matching.compare_faces(e[pr3], gallery, 1e9)
    d0, d3 = float((e[pr3] - e[first0]).norm()), float((e[pr3] - e[en3]).norm())
    assert (name, idx) == (("class3", 1) if d3 < d0 else ("class0", 0)) and abs(dist - min(d0, d3)) <= 1e-4 * max(1.0, min(d0, d3))
    assert d3 < d0                                      # the fitted embedding puts a class-3 probe next to class 3


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


def test_fit_pair_head_end_to_end(tmp_path, calibrated_sd):
    """`fit_pair_head(layer="fc_hidden")` for three epochs on a SiameseNet: a [256, 512] head, the model's own fc.8.  After `load_into`
    the model's embedding (fp16 compute) against `head.embed(model.fc_hidden_features(x))`: 1 - cos <= 1e-3, the project's stated fp16
    bound; `evaluate.siamese_verify` runs on the fitted model."""
    import frmap_amd
    from frmap_amd import evaluate
    root = _folder(str(tmp_path / "faces"))
    model = frmap_amd.get_model("siamese", 36)
    model.load_state_dict(calibrated_sd("siamese"))
    model = model.to(DEV).eval().set_compute_dtype(torch.float16)
    x = next(evaluate._folder_batches(evaluate.image_folder(root)[0], 8, DEV))[0]
    with torch.no_grad():
        hidden = model.fc_hidden_features(x)
        assert hidden.shape == (8, 512) and hidden.dtype == torch.float32 and float(hidden.min()) >= 0.0
    feats, labels = hf.cache_embeddings(model, root, layer="fc_hidden")
    assert feats.shape == (32, 512) and sorted(labels.tolist()) == [c for c in range(4) for _ in range(8)]
    emb_cache, _ = hf.cache_embeddings(model, root)
    assert emb_cache.shape == (32, 256)
    head, hist = hf.fit_pair_head(model, root, val_data=root, epochs=3, batch_pairs=16, lr=1e-3, layer="fc_hidden",
                                  generator=torch.Generator().manual_seed(3))
    print("fit_pair_head: train loss %s acc %s val eer %s" % (["%.4f" % v for v in hist["train_loss"]], ["%.2f" % v for v in hist["train_acc"]],
                                                            ["%.3f" % m["eer"] for m in hist["val"]]))
    assert isinstance(head, hf.PairHead) and (head.D, head.E) == (512, 256) and len(hist["train_loss"]) == 3 and len(hist["val"]) == 3
    assert hist["train_loss"][-1] < hist["train_loss"][0]
    fig = head.epoch_figures()
    assert fig["rows"] == 2 * 16 and fig["t"] == 3 * 2
    before = model.get_embedding(x).float().clone()
    head.load_into(model)
    with torch.no_grad():
        got = model.get_embedding(x).float()
        want = head.embed(model.fc_hidden_features(x))
    cos = torch.nn.functional.cosine_similarity(got, want, dim=1)
    print("siamese after load_into: 1 - cos max %.3g" % float((1 - cos).max()))
    assert not torch.equal(before, got), "load_into did not change the model's embedding"
    assert float((1 - cos).max()) <= 1e-3
    assert torch.equal(model.fc[8].weight.detach(), head.weight) and torch.equal(model.fc[8].bias.detach(), head.bias)
    dist, pred = evaluate.siamese_verify(model, x[:4], x[4:8])
    assert dist.shape == (4,) and pred.shape == (4,) and bool(torch.isfinite(dist).all())
    with pytest.raises(ValueError, match="no classifier head"):
        hf.fit_head(model, "siamese", root)


def test_fit_pair_head_draws_in_the_documented_order():
    """`fit_pair_head` against the same fit replayed by hand, N = 20, D = 8, E = 5, 8 pairs a step (ceil(20 / 8) = 3 steps an epoch),
    2 epochs, dropout 0.25: the device generator's seed from the CPU generator FIRST, then the head from it (the reverse of `fit_head`);
    per step `draw_pairs` (one `randint`, one `rand((3, P))`), then the mask's `rand((2P, D))`; `head.step`.  Weight, bias, the whole
    state and the history are equal."""
    from test_head_fit_gpu import _FlatTrunk
    rng = np.random.default_rng(9)
    data = [(torch.from_numpy(rng.standard_normal((n, 2, 2, 2)).astype(F32)), torch.from_numpy(rng.integers(0, 3, n))) for n in (12, 8)]
    data[0][1][:3] = torch.tensor([0, 1, 2])
    trunk, kw = _FlatTrunk(), dict(lr=1e-2, weight_decay=1e-4, decoupled=True)
    epochs, P, dropout, E = 2, 8, 0.25, 5
    got, hist = hf.fit_pair_head(trunk, data, epochs=epochs, batch_pairs=P, dropout=dropout, embed_dim=E, amsgrad=True, device=DEV,
                                 generator=torch.Generator().manual_seed(21), **kw)
    feats, labels = hf.cache_embeddings(trunk, data, device=DEV)
    N, D = feats.shape
    assert (N, D, int(labels.max()) + 1) == (20, 8, 3)
    gen = torch.Generator().manual_seed(21)
    dev_gen = torch.Generator(device=DEV)
    dev_gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=gen).item()))
    head = hf.PairHead(D, E, DEV, amsgrad=True, generator=gen)
    want = {"train_loss": [], "train_acc": [], "val": []}
    sizes = []
    for _ in range(epochs):
        head.new_epoch()
        for _ in range((N + P - 1) // P):
            left, right, differ = hf.draw_pairs(labels, P, dev_gen)
            sizes.append(int(left.shape[0]))
            keep = (torch.rand((2 * P, D), device=DEV, generator=dev_gen) >= dropout).to(torch.uint8)
            head.step(feats, left, right, differ, keep, dropout=dropout, **kw)
        fig = head.epoch_figures()
        want["train_loss"].append(fig["loss"])
        want["train_acc"].append(fig["accuracy"])
    assert sizes == [8, 8, 8] * epochs
    assert type(got) is type(head)
    for name in ("weight", "bias", "state"):
        assert torch.equal(getattr(got, name), getattr(head, name)), name
    assert hist == want and len(hist["train_loss"]) == epochs and got.epoch_figures()["t"] == 3 * epochs
