"""GPU: the head-fitting step (`frmap_head_fit_step`, csrc/head_fit.hip) against its host twin, and `head_fit.fit_head` end to end.

Every step of every case is compared four ways (`_compare_step`):
  * z holds the bits of the twin's z (the twin's forward from the same weights): the MFMA tiles and the fmaf edges follow the
    rule's chain order;
  * g and the row loss against the float64 softmax of the device's OWN z, gated at 4 x the worst deviation a float32 numpy
    restatement of a wavefront's summation order shows on the same logits (`fit_cases.softmax32`; the tally's convention) and no
    floor: the kernel evaluates the softmax in float64 and rounds once, so it sits at half a unit in the last place where a
    float32 evaluation sits at several.  The figures are printed; the worst measured on an MI355X are in DESIGN.md;
  * w, b and the WHOLE state - t, n, rows, correct, loss_q, m, v, vmax - hold the bits of the twin run on the device's own z, g
    and row losses (`given_g`);
  * row_src equals the twin's.
"""
import os

import numpy as np
import pytest
import torch

import fit_cases as fc
import guard
from frmap_amd import head_fit as hf

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
WORST = {"g": 0.0, "loss": 0.0}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d bytes differ, first at byte %d" % (what, bad.size, int(bad[0]))


def _to(t, dtype=None):
    return None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(DEV)


def _kw(var):
    return dict(fc.HYPER, label_smoothing=var["label_smoothing"], decoupled=var["decoupled"], amsgrad=var["amsgrad"])


def _compare_step(x, labels, rows, keep, keep_scale, w, b, st, dev, var, what, clear=False, B=None):
    """One device step from host state (w, b, st) - updated in place to the device's - with the four comparisons."""
    B = B if B is not None else len(rows) if rows is not None else (len(keep) if keep is not None else len(x))
    D, C = x.shape[1], w.shape[0]
    xd, ld, rd, kd, wd, bd, sd, wsd = dev
    kw = _kw(var)
    hf.step(xd, ld, wd, bd, sd, wsd, rd, kd, keep_scale, clear=clear, batch=B, **kw)
    ws_dev = wsd.cpu().numpy()
    got = hf.workspace_views(ws_dev, B, C)
    # the twin's own forward
    wt, bt, stt = w.copy(), b.copy(), st.copy()
    tw = hf.workspace_views(hf.step_host(x, labels, wt, bt, stt, None, rows, keep, keep_scale, clear=clear, batch=B, **kw), B, C)
    _same(got["row_src"], tw["row_src"], what + ": row_src")
    _same(got["z"], tw["z"], what + ": z")
    ok = got["row_src"] >= 0
    n = int(ok.sum())
    assert np.isnan(got["row_loss"][~ok]).all() and not got["g"][~ok].any() and not got["z"][~ok].any(), what
    if n:
        y = labels[got["row_src"][ok]]
        g64, l64 = fc.softmax64(got["z"][ok], y, n, var["label_smoothing"], C)
        g32, l32 = fc.softmax32(got["z"][ok], y, n, var["label_smoothing"], C)
        g_gate, l_gate = 4.0 * float(np.abs(g32 - g64).max()), 4.0 * float(np.abs(l32 - l64).max())
        g_err, l_err = float(np.abs(got["g"][ok] - g64).max()), float(np.abs(got["row_loss"][ok] - l64).max())
        print("%s: g err %.3g (gate %.3g) | loss err %.3g (gate %.3g)" % (what, g_err, g_gate, l_err, l_gate))
        for k, v in (("g", float((np.abs(got["g"][ok] - g64) / fc.ulp32(g64)).max())), ("loss", float((np.abs(got["row_loss"][ok] - l64) / fc.ulp32(l64)).max()))):
            WORST[k] = max(WORST[k], v)
        assert g_err <= g_gate and l_err <= l_gate, (what, g_err, g_gate, l_err, l_gate)
    # the twin on the device's own z, g and row losses
    hf.step_host(x, labels, w, b, st, ws_dev.copy(), rows, keep, keep_scale, clear=clear, given_g=True, batch=B, **kw)
    _same(wd.cpu().numpy(), w, what + ": w")
    _same(bd.cpu().numpy(), b, what + ": b")
    sdev = sd.cpu().numpy()
    hv, tv = hf.state_views(sdev, D, C, var["amsgrad"]), hf.state_views(st, D, C, var["amsgrad"])
    for name in tv:
        _same(hv[name], tv[name], what + ": state." + name)
    _same(sdev, st, what + ": state")
    return got


def _device(x, labels, rows, keep, w, b, st, B):
    D, C = x.shape[1], w.shape[0]
    return (_to(x), _to(labels), _to(rows), _to(keep), _to(w), _to(b), _to(st),
            torch.empty((hf.workspace_bytes(B, D, C),), dtype=torch.uint8, device=DEV))


def _run_case(seed, B, D, C, var, steps, declined=True):
    x, labels, w, b, rows, keep = fc.problem(seed, B, D, C, declined, var["rows"], var["keep"])
    st = np.zeros((hf.state_bytes(D, C, var["amsgrad"]),), np.uint8)
    dev = _device(x, labels, rows, keep, w, b, st, B)
    for s in range(steps):
        _compare_step(x, labels, rows, keep, 1.0 / 0.75, w, b, st, dev, var, "B=%d D=%d C=%d %s step %d" % (B, D, C, var, s), clear=s == 0, B=B)
    fig = hf.figures_of({k: hf.state_views(st, D, C, var["amsgrad"])[k] for k in hf.HEADER})
    assert fig["rows"] == steps * int(hf.state_views(st, D, C, var["amsgrad"])["n"]) and int(hf.state_views(st, D, C, var["amsgrad"])["t"]) == steps


@pytest.mark.parametrize("B", fc.SWEEP_B)
def test_kernel_against_the_twin(B):
    for D in fc.SWEEP_D:
        for C in fc.SWEEP_C:
            idx = fc.shapes().index((B, D, C))
            _run_case(100 + idx, B, D, C, fc.variation(idx), fc.STEPS)
    print("worst so far, in float32 units in the last place of the float64 value: g %.3g, loss %.3g" % (WORST["g"], WORST["loss"]))


@pytest.mark.parametrize("B,D,C", fc.TILE_EDGES)
def test_tile_edges(B, D, C):
    _run_case(7, B, D, C, {"rows": True, "keep": True, "amsgrad": True, "decoupled": False, "label_smoothing": 0.05}, 1)


def _plain_steps(x, labels, rows, keep, w, b, var, steps=1, st=None):
    """`steps` device steps from (w, b, st); returns the device's (w, b, state, workspace) as numpy."""
    B = len(rows) if rows is not None else (len(keep) if keep is not None else len(x))
    st = np.zeros((hf.state_bytes(x.shape[1], w.shape[0], var["amsgrad"]),), np.uint8) if st is None else st
    xd, ld, rd, kd, wd, bd, sd, wsd = _device(x, labels, rows, keep, w, b, st, B)
    for _ in range(steps):
        hf.step(xd, ld, wd, bd, sd, wsd, rd, kd, 1.0 / 0.75, **_kw(var))
    return wd.cpu().numpy(), bd.cpu().numpy(), sd.cpu().numpy(), wsd.cpu().numpy()


def test_determinism_and_rows_as_a_view():
    B, D, C = 200, 130, 37
    var = fc.variation(1 | 2 | 4 | 16)
    x, labels, w, b, rows, keep = fc.problem(11, B, D, C, declined=False)
    one, two = _plain_steps(x, labels, rows, keep, w, b, var, 2), _plain_steps(x, labels, rows, keep, w, b, var, 2)
    for a, c, name in zip(one, two, ("w", "b", "state", "workspace")):
        _same(a, c, "the same two steps twice: " + name)
    # `rows` as a permutation of the cache = the gathered copy without `rows`
    gathered = _plain_steps(np.ascontiguousarray(x[rows]), np.ascontiguousarray(labels[rows]), None, keep, w, b, var, 2)
    B_, C_ = B, C
    for a, c, name in zip(one[:3], gathered[:3], ("w", "b", "state")):
        _same(a, c, "rows as a view against the gathered copy: " + name)
    va, vg = hf.workspace_views(one[3], B_, C_), hf.workspace_views(gathered[3], B_, C_)
    for name in ("z", "g", "row_loss"):
        _same(va[name], vg[name], "rows as a view against the gathered copy: " + name)
    assert np.array_equal(va["row_src"], rows) and np.array_equal(vg["row_src"], np.arange(B))


def test_a_nan_feature_declines_only_its_row():
    B, D, C = 70, 96, 10
    var = fc.variation(4)
    x, labels, w, b, _, _ = fc.problem(12, B, D, C, declined=False, rows=False, keep=False)
    x, labels = x[:B].copy(), labels[:B].copy()
    bad = x.copy()
    bad[33, 95] = np.nan
    without = np.delete(np.arange(B), 33).astype(np.int32)
    a = _plain_steps(bad, labels, None, None, w, b, var)
    c = _plain_steps(x, labels, without, None, w, b, var)
    for p, q, name in zip(a[:2], c[:2], ("w", "b")):
        _same(p, q, "a NaN row against the batch without it: " + name)
    va, vc = hf.workspace_views(a[3], B, C), hf.workspace_views(c[3], B - 1, C)
    assert va["row_src"][33] == -1 and (np.delete(va["row_src"], 33) == without).all() and np.isnan(va["row_loss"][33])
    _same(np.delete(va["z"], 33, axis=0), vc["z"], "z of the other rows")
    _same(np.delete(va["g"], 33, axis=0), vc["g"], "g of the other rows")
    ha, hc = hf.state_views(a[2], D, C, True), hf.state_views(c[2], D, C, True)
    assert int(ha["n"]) == int(hc["n"]) == B - 1 and int(ha["t"]) == 1
    # every row declined: nothing moves
    allbad = x.copy()
    allbad[:, 0] = np.inf
    w2, b2, st2, ws2 = _plain_steps(allbad, labels, None, None, w, b, var)
    _same(w2, w, "all rows declined: w")
    _same(b2, b, "all rows declined: b")
    assert not st2.any() and (hf.workspace_views(ws2, B, C)["row_src"] == -1).all()


def test_guard_bands_at_element_alignment():
    """Every buffer at its element alignment (fp32 / int32 4, keep 1, state 8, workspace 4: aligned to that and not to twice
    that), the workspace exactly `workspace_bytes`, under fills 0xFF and 0x5A: the bands and the read-only operands stay untouched
    and the results are identical under both fills and equal to the unguarded call."""
    B, D, C = 45, 70, 35
    var = fc.variation(1 | 2 | 4 | 16)
    x, labels, w, b, rows, keep = fc.problem(13, B, D, C)
    ref = _plain_steps(x, labels, rows, keep, w, b, var)
    need = {"state": 8, "workspace": 4, "w": 4, "b": 4}
    results = []
    for fill in guard.FILLS:
        g = guard.Guard(fill, device=DEV, shift=guard.min_placement(
            lambda dtype, kind, who: need.get(who, 1 if dtype == torch.uint8 else 4)))
        xd, ld, rd, kd = (g.place(torch.from_numpy(t)) for t in (x, labels, rows, keep))
        wd, bd = g.empty(w.shape, torch.float32, "w"), g.empty(b.shape, torch.float32, "b")
        sd = g.empty((hf.state_bytes(D, C, True),), torch.uint8, "state")
        wsd = g.empty((hf.workspace_bytes(B, D, C),), torch.uint8, "workspace")
        assert sd.data_ptr() % 16 == 8 and wsd.data_ptr() % 8 == 4 and wd.data_ptr() % 8 == 4 and kd.data_ptr() % 2 == 1
        wd.copy_(torch.from_numpy(w))
        bd.copy_(torch.from_numpy(b))
        sd.zero_()
        hf.step(xd, ld, wd, bd, sd, wsd, rd, kd, 1.0 / 0.75, **_kw(var))
        g.check()
        results.append((wd.cpu().numpy(), bd.cpu().numpy(), sd.cpu().numpy(), wsd.cpu().numpy()))
    for k, name in enumerate(("w", "b", "state", "workspace")):
        _same(results[0][k], results[1][k], "fill 0xFF against fill 0x5A: " + name)
        _same(results[0][k], ref[k], "guarded against unguarded: " + name)


def test_a_captured_step_replays():
    """A captured step (one stream, no branches) replayed twice = two eager steps: t lives in the state."""
    B, D, C = 64, 128, 18
    var = fc.variation(1 | 2)
    x, labels, w, b, rows, keep = fc.problem(14, B, D, C)
    eager = _plain_steps(x, labels, rows, keep, w, b, var, 2)
    st = np.zeros((hf.state_bytes(D, C, False),), np.uint8)
    xd, ld, rd, kd, wd, bd, sd, wsd = _device(x, labels, rows, keep, w, b, st, B)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            hf.step(xd, ld, wd, bd, sd, wsd, rd, kd, 1.0 / 0.75, **_kw(var))
        wd.copy_(torch.from_numpy(w))                 # (capture does not run the step; start from the same weights anyway)
        bd.copy_(torch.from_numpy(b))
        sd.zero_()
        graph.replay()
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    for a, c, name in zip(eager, (wd.cpu().numpy(), bd.cpu().numpy(), sd.cpu().numpy(), wsd.cpu().numpy()), ("w", "b", "state", "workspace")):
        _same(a, c, "two replays against two eager steps: " + name)
    assert int(hf.state_views(eager[2], D, C)["t"]) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _folder(root, classes=4, per_class=8, seed=5):
    """A synthetic image folder whose trunk features are separable BY CONSTRUCTION: every class is one random base image (a 4 x 4
    grid of saturated colours, so the classes differ in large uniform patches that survive the trunk's pooling) and its samples
    are that image plus noise of a tenth of its contrast.  32 samples of 512 features are linearly separable whenever they are in
    general position; the shared base makes the margin wide, so that Adam finds it in few epochs."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    for c in range(classes):
        os.makedirs(os.path.join(root, "class%d" % c))
        base = np.kron(rng.integers(0, 2, (4, 4, 3)) * 200.0 + 25.0, np.ones((16, 16, 1)))
        for k in range(per_class):
            img = np.clip(base + rng.normal(0, 20.0, base.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, "class%d" % c, "img%d.png" % k))
    return root


def _model(mt, sd):
    import frmap_amd
    m = frmap_amd.get_model(mt, 36)
    m.load_state_dict(sd)
    return m.to(DEV).eval().set_compute_dtype(torch.float16)


def test_fit_head_end_to_end(tmp_path, calibrated_sd):
    from frmap_amd import evaluate
    root = _folder(str(tmp_path / "faces"))
    model = _model("cnn", calibrated_sd("cnn"))
    gen = torch.Generator().manual_seed(3)
    head, hist = hf.fit_head(model, "cnn", root, val_data=root, epochs=30, batch_size=8, lr=1e-2, generator=gen, num_classes=36)
    print("fit_head cnn: train loss %s\n train acc %s" % (["%.3f" % v for v in hist["train_loss"]], ["%.2f" % v for v in hist["train_acc"]]))
    assert len(hist["train_loss"]) == 30 and len(hist["val"]) == 30
    assert max(hist["train_acc"]) == 1.0 and hist["train_acc"][-1] == 1.0, hist["train_acc"]
    assert hist["train_loss"][-1] < hist["train_loss"][0]
    assert hist["val"][-1]["accuracy"] == 1.0 and hist["val"][-1]["rows"] == 32
    fig = head.epoch_figures()
    assert fig["rows"] == 32 and fig["t"] == 30 * 4
    # the fitted head inside the model: forward() = the head on the model's own embedding (test_models_gpu.TOL: relative L2 1.5e-2)
    feats, labels = hf.cache_features(model, "cnn", root)
    before = model(evaluate.preprocess(torch.zeros((2, 224, 224, 3), dtype=torch.uint8, device=DEV), device=DEV)).clone()
    head.load_into(model)
    x = next(evaluate._folder_batches(evaluate.image_folder(root)[0], 8, DEV))[0]
    with torch.no_grad():
        out, want = model(x).float(), head.logits(model.get_embedding(x).float())
    rel = float((out - want).norm() / want.norm())
    print("load_into: relative L2 of model(x) against head.logits(get_embedding(x)) %.3g" % rel)
    assert rel < 1.5e-2 and out.shape == (8, 36) and out.argmax(1).tolist() == [0] * 8
    assert not torch.equal(before, model(evaluate.preprocess(torch.zeros((2, 224, 224, 3), dtype=torch.uint8, device=DEV), device=DEV)))
    sd = head.state_dict()
    assert sorted(sd) == ["bias", "weight"] and torch.equal(sd["weight"], model.resnet.fc[1].weight.detach())
    # arcface: a trained head as `arcface_classifier`
    arc = _model("arcface", calibrated_sd("arcface"))
    head2, hist2 = hf.fit_head(arc, "arcface", root, epochs=30, batch_size=8, lr=1e-2, weight_decay=1e-4, dropout=0.0, label_smoothing=0.05,
                               decoupled=True, amsgrad=True, generator=gen, num_classes=4)
    f2, l2 = hf.cache_features(arc, "arcface", root)
    head2.new_epoch().step(f2, l2, lr=0.0)                     # lr 0: the figures of the final weights, which do not move
    own = head2.epoch_figures()
    m = evaluate.evaluate_stream(arc, "arcface", root, arcface_classifier=head2.as_classifier(), device=DEV)
    print("arcface head: own accuracy %.3f over %d rows, evaluate_stream %.3f" % (own["accuracy"], own["rows"], m["accuracy"]))
    assert own["rows"] == m["rows"] == 32 and m["accuracy"] == own["accuracy"] and hist2["train_acc"][-1] >= 0.9
    with pytest.raises(ValueError, match="siamese"):
        hf.fit_head(None, "siamese", root)


class _FlatTrunk:
    """A trunk by duck typing (not a ``BaselineNet``): the embedding of an image is the image, flattened."""
    training = False

    def eval(self):
        return self

    def get_embedding(self, im):
        return im.reshape(im.shape[0], -1)


@pytest.mark.parametrize("hidden", [None, 5], ids=["linear", "hidden"])
def test_fit_head_draws_in_the_documented_order(hidden):
    """`fit_head` against the same fit replayed by hand, N = 20, D = 8, C = 3, batches of 8 (the last one has 4 rows), 2 epochs: the head
    from the CPU generator, then the device generator's seed from it; per epoch one `randperm`; per batch the input mask's `rand`,
    then (hidden) the hidden mask's; `head.step`.  Every weight, bias, the whole state and the history are equal."""
    rng = np.random.default_rng(9)
    data = [(torch.from_numpy(rng.standard_normal((n, 2, 2, 2)).astype(F32)), torch.from_numpy(rng.integers(0, 3, n))) for n in (12, 8)]
    data[0][1][:3] = torch.tensor([0, 1, 2])
    trunk, kw = _FlatTrunk(), dict(lr=1e-2, weight_decay=1e-4, label_smoothing=0.05, decoupled=True)
    epochs, batch, dropout, hidden_dropout = 2, 8, 0.25, 0.5
    got, hist = hf.fit_head(trunk, "cnn", data, epochs=epochs, batch_size=batch, dropout=dropout, amsgrad=True, device=DEV, hidden=hidden,
                            hidden_dropout=hidden_dropout, generator=torch.Generator().manual_seed(21), **kw)
    feats, labels = hf.cache_features(trunk, "cnn", data, device=DEV)
    N, D = feats.shape
    assert (N, D, int(labels.max()) + 1) == (20, 8, 3)
    gen = torch.Generator().manual_seed(21)
    if hidden is None:
        head = hf.LinearHead(D, 3, DEV, amsgrad=True, generator=gen)
    else:
        head = hf.HiddenHead(D, hidden, 3, DEV, amsgrad=True, generator=gen)
    dev_gen = torch.Generator(device=DEV)
    dev_gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=gen).item()))
    want = {"train_loss": [], "train_acc": [], "val": []}
    sizes = []
    for _ in range(epochs):
        perm = torch.randperm(N, device=DEV, generator=dev_gen).to(torch.int32)
        head.new_epoch()
        for lo in range(0, N, batch):
            rows = perm[lo: lo + batch]
            sizes.append(int(rows.shape[0]))
            keep = (torch.rand((rows.shape[0], D), device=DEV, generator=dev_gen) >= dropout).to(torch.uint8)
            if hidden is None:
                head.step(feats, labels, rows, keep, dropout=dropout, **kw)
            else:
                keep2 = (torch.rand((rows.shape[0], hidden), device=DEV, generator=dev_gen) >= hidden_dropout).to(torch.uint8)
                head.step(feats, labels, rows, keep, keep2, dropout1=dropout, dropout2=hidden_dropout, **kw)
        fig = head.epoch_figures()
        want["train_loss"].append(fig["loss"])
        want["train_acc"].append(fig["accuracy"])
    assert sizes == [8, 8, 4] * epochs
    assert type(got) is type(head)
    for name in ("weight", "bias", "state") if hidden is None else ("w1", "b1", "w2", "b2", "state"):
        assert torch.equal(getattr(got, name), getattr(head, name)), name
    assert hist == want and len(hist["train_loss"]) == epochs and got.epoch_figures()["t"] == 3 * epochs
