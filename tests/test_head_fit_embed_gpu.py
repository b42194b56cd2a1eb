"""GPU: the embedding head-fitting step (`frmap_head_fit_embed_step`, csrc/head_fit_embed.hip) and what is built on it.

THE CONTRACT (`test_kernels_against_the_twin`): over the shapes of `fit_embed_cases.SHAPES` at each of three steps, and for one step at
the two large shapes, every float64 stage of the kernels - mean32, rstd, uvar, ah; the margin stage's rx, rw, cosv, g, h and row loss;
da - is within one fp32 unit in the last place of the float64 value computed from the device's own inputs to that stage, and
everything else - a, lab, row_src1, n1, y', z, gy, dbeta, dgamma, the six parameter tensors and every byte of the state - equals the
host twin's run with ``given = 7`` on the device's stage outputs, bit for bit.  Around it: the margin half against the margin step's
own kernels, determinism, `rows` as a view, declined rows and NaNs, the all-or-nothing cases, guard bands at element alignment, graph
replay on changed inputs, and `fit_embed_head` on an ``ArcFaceNet`` through `load_into`, `evaluate_stream` and the model handle."""
import numpy as np
import pytest
import torch

import fit_embed_cases as ec
import fit_margin_cases as mc
import guard
from frmap_amd import head_fit as hf
from test_head_fit_embed_cpu import MARGIN_GIVEN, STAGE1, STAGE3, exact_stages
from test_head_fit_margin_cpu import ROUNDED, exact_halves, within_one_ulp
from test_head_fit_margin_gpu import _folder, _same, _to

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
OUT = ec.PARAMS + ("state", "workspace")


class _Device:
    """A problem's operands on the device, from host arrays."""

    def __init__(self, p, var, fill=None):
        B, D, E, C = p["B"], p["D"], p["E"], p["C"]
        self.p, self.var = p, var
        self.x, self.labels, self.rows, self.keep = (_to(p[k]) for k in ("x", "labels", "rows", "keep"))
        self.params = {n: _to(p[n]) for n in ec.PARAMS}
        self.st = torch.zeros((hf.embed_state_bytes(D, E, C, var["amsgrad"]),), dtype=torch.uint8, device=DEV)
        self.ws = torch.empty((hf.embed_workspace_bytes(B, D, E, C),), dtype=torch.uint8, device=DEV)
        if fill is not None:
            self.ws.fill_(fill)

    def step(self, k, clear=None, **over):
        hf.embed_step(self.x, self.labels, *[self.params[n] for n in ec.PARAMS], self.st, self.ws, self.rows, self.keep,
                      ec.keep_scale(self.var) if self.keep is not None else 1.0, batch=self.p["B"], **dict(ec.step_kw(self.var, k, clear), **over))

    def host(self):
        return [self.params[n].cpu().numpy() for n in ec.PARAMS] + [self.st.cpu().numpy(), self.ws.cpu().numpy()]


def _run(p, var, steps=ec.STEPS, fill=None, **over):
    d = _Device(p, var, fill)
    for k in range(steps):
        d.step(k, **over)
    return d.host()


def _twin(p, var, kw, params, st, ws, given):
    return hf.embed_step_host(p["x"], p["labels"], *[params[n] for n in ec.PARAMS], st, ws, p["rows"], p["keep"],
                              ec.keep_scale(var) if p["keep"] is not None else 1.0, given=given, batch=p["B"], **kw)


def _contract(shape, steps):
    """The contract on one shape.  Returns the worst deviation of every float64 stage, in units in the last place."""
    B, D, E, C = shape
    var = ec.variation(shape)
    p = ec.problem(ec.case_seed(shape), *shape, var)
    d = _Device(p, var, 0x5A)
    tp, stt = ec.params_of(p), np.zeros(d.st.numel(), np.uint8)
    worst = dict.fromkeys(STAGE1 + STAGE3 + ROUNDED, 0.0)
    for k in steps:
        what = "%s step %d" % (ec.case_id(shape), k)
        kw = ec.step_kw(var, k)
        before = {n: v.copy() for n, v in tp.items()}
        d.step(k)
        got = d.host()
        gws = got[-1]
        v = hf.embed_workspace_views(gws, B, E, C)
        n1 = int(v["n1"][0])
        assert n1 == B
        exact = exact_stages(p, v, before, kw, n1)
        for name in STAGE1 + STAGE3:
            worst[name] = max(worst[name], within_one_ulp(v[name], exact[name], what + ": " + name))
        mkw = {a: b for a, b in kw.items() if a not in ("bn_eps", "bn_momentum")}
        mexact = exact_halves(v["yp"], v["lab"], before["wc"], v["margin"], None, None, 1.0, dict(mkw, batch=B))
        for name in ROUNDED:
            worst[name] = max(worst[name], within_one_ulp(v["margin"][name], mexact[name], what + ": margin " + name))
        tws = gws.copy()
        _twin(p, var, kw, tp, stt, tws, 7)
        _same(tws, gws, what + ": the workspace of the twin with given = 7")
        for n, g in zip(ec.PARAMS, got):
            _same(g, tp[n], what + ": " + n)
        _same(got[-2], stt, what + ": the state")
    views = hf.embed_state_views(got[-2], D, E, C, var["amsgrad"])
    assert all(int(views[part]["t"]) == len(steps) and int(views[part]["n"]) == B for part in views)
    return worst


@pytest.mark.parametrize("group", range(0, len(ec.SHAPES), 4))
def test_kernels_against_the_twin(group):
    """The shape table, four shapes a test, three steps each."""
    worst = dict.fromkeys(STAGE1 + STAGE3 + ROUNDED, 0.0)
    for shape in ec.SHAPES[group: group + 4]:
        for name, v in _contract(shape, tuple(range(ec.STEPS))).items():
            worst[name] = max(worst[name], v)
    print("kernels against the twin, shapes %d..: worst units in the last place %s" % (group, {k: round(v, 3) for k, v in worst.items()}))


@pytest.mark.parametrize("shape", ec.BIG_SHAPES, ids=ec.case_id)
def test_kernels_against_the_twin_at_the_deployed_shapes(shape):
    """One step (step 2: AMSGrad or a mask, smoothing, the full margin) at the shapes of the deployed model."""
    worst = _contract(shape, (2,))
    print("kernels against the twin, %s: worst units in the last place %s" % (ec.case_id(shape), {k: round(v, 3) for k, v in worst.items()}))


def test_the_margin_half_is_the_margin_step_kernel_against_kernel():
    """`margin_step` on clones of y', lab, the centres and the margin part of the state from before the step: the margin workspace, the
    centres and the margin state of the embedding step are its bytes."""
    for shape in ((33, 31, 33, 18), (40, 5, 130, 35)):
        B, D, E, C = shape
        var = ec.variation(ec.SHAPES[1])
        p = ec.problem(4100, *shape, var)
        d = _Device(p, var)
        at, n = hf.embed_state_parts(D, E, C, var["amsgrad"])["margin"]
        for k in range(2):
            wc0, st3 = d.params["wc"].clone(), d.st[at: at + n].clone()
            d.step(k)
            v = hf.embed_workspace_views(d.ws.cpu().numpy(), B, E, C)
            mws = torch.empty((hf.margin_workspace_bytes(B, E, C),), dtype=torch.uint8, device=DEV)
            kw = {a: b for a, b in ec.step_kw(var, k).items() if a not in ("bn_eps", "bn_momentum")}
            hf.margin_step(_to(v["yp"]), _to(v["lab"]), wc0, st3, mws, **kw)
            off = d.ws.numel() - mws.numel()
            _same(d.ws[off:], mws, "step %d: the margin workspace" % k)
            _same(d.params["wc"], wc0, "step %d: the centres" % k)
            _same(d.st[at: at + n], st3, "step %d: the margin state" % k)


def test_two_runs_give_the_same_bytes():
    shape = (257, 33, 65, 130)
    var = ec.VARIATIONS[0]
    p = ec.problem(4200, *shape, var)
    a, b = _run(p, var, 2, 0xFF), _run(p, var, 2, 0x5A)
    for u, v, name in zip(a, b, OUT):
        _same(u, v, "two runs: " + name)


def test_rows_as_a_view_against_the_gathered_copy():
    shape = (40, 33, 35, 18)
    var = ec.VARIATIONS[0]
    p = ec.problem(4300, *shape, var)
    gathered = dict(p, x=p["x"][p["rows"]].copy(), labels=p["labels"][p["rows"]].copy(), rows=None, N=shape[0])
    for u, v, name in zip(_run(p, var, 2), _run(gathered, var, 2), OUT):
        if name == "workspace":
            a, b = hf.embed_workspace_views(u, 40, 35, 18), hf.embed_workspace_views(v, 40, 35, 18)
            for key in ("a", "ah", "yp", "gy", "da", "mean32", "rstd", "uvar", "dbeta", "dgamma", "lab"):
                _same(a[key], b[key], "rows as a view: " + key)
        else:
            _same(u, v, "rows as a view: " + name)


@pytest.mark.parametrize("kind", ("row -1", "label C", "nan feature"))
def test_a_declined_row_counts_for_nothing(kind):
    """A declined row inserted into the batch (a NaN feature included: the NaN reaches nothing): parameters and state are those of the
    batch without it."""
    shape = (33, 31, 33, 18)
    var = ec.VARIATIONS[1]
    p = ec.problem(4400, *shape, var)
    q = ec.with_bad_row(p, kind, 7)
    a, b = _run(p, var, 2), _run(q, var, 2)
    for u, v, name in zip(a[:-1], b[:-1], OUT[:-1]):
        _same(u, v, kind + ": " + name)
    vb = hf.embed_workspace_views(b[-1], 34, 33, 18)
    assert vb["row_src1"][7] == -1 and vb["lab"][7] == -1 and int(vb["n1"][0]) == 33 and not np.isnan(b[0]).any()
    for name in ("a", "ah", "yp", "gy", "da"):
        assert not vb[name][7].any(), name


@pytest.mark.parametrize("case", ("B1", "two of three declined", "nan in w1", "nan in gamma"))
def test_all_or_nothing(case):
    """A step that is not taken - from a fresh state and after a good step - leaves every byte of the parameters and the state (word n
    of the three headers is the count of the step in flight: 0 after it) and equals the twin's workspace handling: da is +0."""
    var = ec.VARIATIONS[1]
    B = 1 if case == "B1" else 3
    p = ec.problem(321, B, 5, 4, 3, var)
    good = ec.problem(321, 6, 5, 4, 3, var)
    if case == "two of three declined":
        p["rows"] = np.array([p["rows"][0], -1, p["N"]], np.int32)
    for after_good in (False, True):
        d = _Device(p, var, 0xFF)
        if after_good:
            g = _Device(good, var)
            g.step(0)
            d.st.copy_(g.st)
            for n in ec.PARAMS:
                d.params[n].copy_(g.params[n])
        if case == "nan in w1":
            d.params["w1"][2, 1] = float("nan")
        if case == "nan in gamma":
            d.params["gamma"][1] = float("nan")
        before = d.host()
        d.step(1, clear=False)
        got = d.host()
        for u, v, name in zip(before[:-2], got[:-2], OUT[:-2]):
            _same(u, v, case + ": " + name)
        views, was = hf.embed_state_views(got[-2], 5, 4, 3, True), hf.embed_state_views(before[-2], 5, 4, 3, True)
        for part in views:
            assert int(views[part]["n"]) == 0 and int(views[part]["t"]) == (1 if after_good else 0), part
            was[part]["n"][...] = 0
        _same(before[-2], got[-2], case + ": the state")
        v = hf.embed_workspace_views(got[-1], B, 4, 3)
        assert not v["da"].any() and int(v["n1"][0]) == (1 if case in ("B1", "two of three declined") else 3)


def test_guard_bands_at_element_alignment():
    """Every operand between guard bands at its element alignment (fp32 / int32 4, the mask 1, the state 8, the workspace 4: aligned to
    that and not to twice that), the state and the workspace at exactly their reported sizes, under fills 0xFF and 0x5A: the bands and
    the read-only operands stay untouched, and the results are identical under both fills and equal to the unguarded call."""
    for shape in ((23, 70, 35, 33), (3, 2, 3, 2), (40, 33, 130, 5)):
        B, D, E, C = shape
        var = dict(ec.VARIATIONS[1], keep=True)
        p = ec.problem(4500, *shape, var)
        need = dict({n: 4 for n in ec.PARAMS}, state=8, workspace=4)
        results = []
        for fill in guard.FILLS:
            g = guard.Guard(fill, device=DEV, shift=guard.min_placement(lambda dtype, kind, who: need.get(who, 1 if dtype == torch.uint8 else 4)))
            xd, ld, rd, kd = (g.place(torch.from_numpy(p[k])) for k in ("x", "labels", "rows", "keep"))
            pd = {n: g.empty(p[n].shape, torch.float32, n) for n in ec.PARAMS}
            sd = g.empty((hf.embed_state_bytes(D, E, C, True),), torch.uint8, "state")
            wsd = g.empty((hf.embed_workspace_bytes(B, D, E, C),), torch.uint8, "workspace")
            assert sd.data_ptr() % 16 == 8 and wsd.data_ptr() % 8 == 4 and pd["gamma"].data_ptr() % 8 == 4 and kd.data_ptr() % 2 == 1
            for n in ec.PARAMS:
                pd[n].copy_(torch.from_numpy(p[n]))
            sd.zero_()
            hf.embed_step(xd, ld, *[pd[n] for n in ec.PARAMS], sd, wsd, rd, kd, ec.keep_scale(var), **ec.step_kw(var, 1, True))
            g.check()
            results.append([pd[n].cpu().numpy() for n in ec.PARAMS] + [sd.cpu().numpy(), wsd.cpu().numpy()])
        d = _Device(p, var)
        d.step(1, clear=True)
        ref = d.host()
        for k, name in enumerate(OUT):
            _same(results[0][k], results[1][k], "B=%d fill 0xFF against fill 0x5A: %s" % (B, name))
            _same(results[0][k], ref[k], "B=%d guarded against unguarded: %s" % (B, name))


def test_a_captured_step_replays_on_changed_inputs():
    """A captured step (one stream, no branches) replayed twice, the cache, the labels, the rows and the mask rewritten on the stream
    between the replays = two eager steps on those inputs: t lives in the state, and the memset of the step in flight replays."""
    shape = (64, 128, 96, 40)
    var = ec.VARIATIONS[0]
    p, q = ec.problem(4600, *shape, var), ec.problem(4601, *shape, var)
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
        for n in ec.PARAMS:                                # (capture does not run the step; start from the same parameters anyway)
            d.params[n].copy_(_to(p[n]))
        d.st.zero_()
        graph.replay()
        for name in names:
            getattr(d, name).copy_(second[name])
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    for a, c, name in zip(eager.host(), d.host(), OUT):
        _same(a, c, "two replays against two eager steps: " + name)
    assert int(hf.embed_state_views(d.st.cpu().numpy(), 128, 96, 40)["margin"]["t"]) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_fit_embed_head_end_to_end(tmp_path, calibrated_sd):
    """`fit_embed_head` for twenty epochs on a calibrated ArcFaceNet over a synthetic folder, four of its 36 classes present.  After
    `load_into` the model's own classification path - `evaluate_stream` - is at least as accurate as before and at 0.9 or better (what
    `test_head_fit_gpu.py` asks of the softmax head on the same folder), and the model's `get_embedding` (the handle route) against
    `head.embed(model.pooled_features(x))` by relative L2 is within 2x what the same comparison reads on the model BEFORE loading,
    with its own embedding and bn - measured first (the hidden head's precedent)."""
    import frmap_amd
    from frmap_amd import evaluate
    root = _folder(str(tmp_path / "faces"))
    model = frmap_amd.get_model("arcface", 36)
    model.load_state_dict(calibrated_sd("arcface"))
    model = model.to(DEV).eval().set_compute_dtype(torch.float16)
    x = next(evaluate._folder_batches(evaluate.image_folder(root)[0], 8, DEV))[0]
    with torch.no_grad():
        pooled = model.pooled_features(x)
        assert pooled.shape == (8, 512) and pooled.dtype == torch.float32
        base = _rel(model.get_embedding(x).float(), hf.EmbedHead.from_model(model).embed(pooled))
    print("arcface before loading: relative L2 of the handle route against pooled_features + EmbedHead.embed: %.3g" % base)
    before = evaluate.evaluate_stream(model, "arcface", root, device=DEV)
    tracked = int(model.bn.num_batches_tracked)
    head, hist = hf.fit_embed_head(model, root, val_data=root, epochs=20, batch_size=8, lr=1e-2, generator=torch.Generator().manual_seed(3))
    print("fit_embed_head: train loss %s acc %s val acc %s" % (["%.3f" % v for v in hist["train_loss"]], ["%.2f" % v for v in hist["train_acc"]],
                                                             ["%.2f" % m["accuracy"] for m in hist["val"]]))
    assert isinstance(head, hf.EmbedHead) and (head.D, head.E, head.C) == (512, 512, 36) and len(hist["train_loss"]) == 20
    fig = head.epoch_figures()
    assert fig["rows"] == 32 and fig["t"] == 20 * 4
    emb_before = model.get_embedding(x).float().clone()
    head.load_into(model)
    assert torch.equal(model.embedding.weight.detach(), head.w1) and torch.equal(model.bn.running_var, head.running_var)
    assert int(model.bn.num_batches_tracked) == tracked + 80
    after = evaluate.evaluate_stream(model, "arcface", root, device=DEV)
    with torch.no_grad():
        got = model.get_embedding(x).float()
        rel = _rel(got, head.embed(model.pooled_features(x)))
    print("arcface after load_into: accuracy %.3f -> %.3f; relative L2 embedding %.3g (bound %.3g)" % (before["accuracy"], after["accuracy"], rel, 2 * base))
    assert not torch.equal(emb_before, got), "load_into did not change the model's embedding"
    assert after["rows"] == 32 and after["accuracy"] >= before["accuracy"] and after["accuracy"] >= 0.9
    assert rel <= 2 * base


class ArcFaceNet(torch.nn.Module):
    """An ``ArcFaceNet`` by name and attributes, as `EmbedHead.from_model` and `cache_features(layer="pooled")` ask: the pooled
    features of an image are the image, flattened to 8; ``embedding`` 8 -> 5 without a bias, ``bn`` over 5, three class centres."""

    def __init__(self):
        super().__init__()
        self.embedding, self.bn = torch.nn.Linear(8, 5, bias=False), torch.nn.BatchNorm1d(5)
        self.arcface = torch.nn.Module()
        self.arcface.weight = torch.nn.Parameter(torch.empty(3, 5).normal_(0.0, 0.5))

    def pooled_features(self, im):
        return im.reshape(im.shape[0], -1)


def test_fit_embed_head_draws_in_the_documented_order():
    """`fit_embed_head` against the same fit replayed by hand, N = 17, D = 8, E = 5, C = 3, batches of 8 (the last one has ONE row: it
    is stepped and the library declines it), 2 epochs, dropout 0.25: no head draw (`EmbedHead.from_model`), then the device generator's
    seed from the CPU generator; per epoch `margin_schedule(epoch)` and one `randperm`; per batch one mask `rand` of ``[rows, E]``;
    `head.step`.  The six tensors, the whole state and the history are equal; ``t`` is 4, and `load_into` advances
    ``num_batches_tracked`` by 4."""
    rng = np.random.default_rng(9)
    data = [(torch.from_numpy(rng.standard_normal((n, 2, 2, 2)).astype(F32)), torch.from_numpy(rng.integers(0, 3, n))) for n in (12, 5)]
    data[0][1][:3] = torch.tensor([0, 1, 2])
    model, kw = ArcFaceNet().to(DEV).eval(), dict(lr=1e-2, weight_decay=1e-4, label_smoothing=0.05, decoupled=True)
    epochs, batch, dropout, s, m = 2, 8, 0.25, 32.0, 0.5
    got, hist = hf.fit_embed_head(model, data, epochs=epochs, batch_size=batch, dropout=dropout, s=s, m=m, amsgrad=True, device=DEV,
                                  generator=torch.Generator().manual_seed(21), **kw)
    feats, labels = hf.cache_features(model, "arcface", data, device=DEV, layer="pooled")
    N, D = feats.shape
    assert (N, D, int(labels.max()) + 1) == (17, 8, 3)
    gen = torch.Generator().manual_seed(21)
    head = hf.EmbedHead.from_model(model, DEV, amsgrad=True)
    assert (head.D, head.E, head.C) == (8, 5, 3)
    dev_gen = torch.Generator(device=DEV)
    dev_gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=gen).item()))
    want = {"train_loss": [], "train_acc": [], "val": []}
    sizes = []
    for epoch in range(epochs):
        m_eff, s_eff = hf.margin_schedule(epoch, s, m)
        perm = torch.randperm(N, device=DEV, generator=dev_gen).to(torch.int32)
        head.new_epoch()
        for lo in range(0, N, batch):
            rows = perm[lo: lo + batch]
            sizes.append(int(rows.shape[0]))
            keep = (torch.rand((rows.shape[0], head.E), device=DEV, generator=dev_gen) >= dropout).to(torch.uint8)
            head.step(feats, labels, rows, keep, s=s_eff, m=m_eff, dropout=dropout, **kw)
        fig = head.epoch_figures()
        want["train_loss"].append(fig["loss"])
        want["train_acc"].append(fig["accuracy"])
    assert sizes == [8, 8, 1] * epochs
    assert type(got) is type(head)
    for name in ("w1", "gamma", "beta", "running_mean", "running_var", "wc", "state"):
        assert torch.equal(getattr(got, name), getattr(head, name)), name
    assert hist == want and len(hist["train_loss"]) == epochs and got.epoch_figures()["t"] == 2 * epochs == 4
    assert hist["train_loss"] and all(np.isfinite(hist["train_loss"])) and got.epoch_figures()["rows"] == 16
    tracked = int(model.bn.num_batches_tracked)
    got.load_into(model)
    assert int(model.bn.num_batches_tracked) == tracked + 4 and torch.equal(model.embedding.weight.detach(), head.w1)
