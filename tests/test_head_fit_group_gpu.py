"""GPU: the grouped head-fitting step (`frmap_head_fit_group_step`, csrc/head_fit.hip) and what is built on it.

THE CONTRACT (`test_group_equals_single_steps_on_cloned_slices`): head h of a grouped step holds exactly the bits of
`frmap_head_fit_step` run on head h's slices alone - z, g, row_loss, row_src, w, b and every state word, device against device, at
each of three steps over `fit_group_cases` - and the group's host twin, run with `given_g` on the device's own z, g and row losses,
gives the device's weights, moments and figures word for word.  Around it: head isolation under NaNs, a head whose rows are all
declined, guard bands at element alignment, graph replay with the hyper table rewritten between replays, operands that arrive
late on a side stream, flag 8, a grid 257 heads deep, head offsets past 2^31 elements, and `cross_validate` / `sweep_heads` against
loops of single `LinearHead` fits."""
import types

import numpy as np
import pytest
import torch

import big_cases
import fit_group_cases as gc
import guard
import stream_cases as sc
from frmap_amd import head_fit as hf, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
CASES = gc.cases()


def _same(a, b, what):
    a = (a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)).view(np.uint8).reshape(-1)
    b = (b.cpu().numpy() if isinstance(b, torch.Tensor) else np.ascontiguousarray(b)).view(np.uint8).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d bytes differ, first at byte %d" % (what, bad.size, int(bad[0]))


def _to(t):
    return None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(DEV)


def _flags(var):
    return dict(decoupled=var["decoupled"], amsgrad=var["amsgrad"])


class _Group:
    """A group's operands on the device, from host arrays."""

    def __init__(self, x, labels, w, b, rows, keep, st, B):
        H, C, D = w.shape
        self.x, self.labels, self.w, self.b, self.rows, self.keep, self.st = (_to(t) for t in (x, labels, w, b, rows, keep, st))
        self.ws = torch.empty((hf.group_workspace_bytes(H, B, D, C),), dtype=torch.uint8, device=DEV)
        self.hyper = torch.zeros((H, 8), dtype=torch.float32, device=DEV)

    def step(self, table, **kw):
        self.hyper.copy_(torch.from_numpy(table))
        hf.group_step(self.x, self.labels, self.rows, self.hyper, self.w, self.b, self.st, self.ws, None if kw.get("evaluate") else self.keep, **kw)

    def host(self):
        return tuple(t.cpu().numpy() for t in (self.w, self.b, self.st, self.ws))


def _run_group(case, seed, steps=gc.STEPS, fill=0, table_of=None):
    """`steps` grouped steps of a case from fresh states; returns the device's (w, b, state, workspace) as numpy."""
    H, B, D, C, var = case
    x, labels, w, b, rows, keep = gc.problem(seed, H, B, D, C, var["keep"], var["dead"])
    g = _Group(x, labels, w, b, rows, keep, gc.fresh_states(H, D, C, var["amsgrad"], fill), B)
    for s in range(steps):
        g.step((table_of or (lambda s_: gc.hyper(H, var["keep"], s_)))(s), clear=s == 0, **_flags(var))
    return g.host()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the contract
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[gc.case_id(c) for c in CASES])
def test_group_equals_single_steps_on_cloned_slices(case):
    H, B, D, C, var = case
    ams = var["amsgrad"]
    x, labels, w, b, rows, keep = gc.problem(2000 + CASES.index(case), H, B, D, C, var["keep"], var["dead"])
    st = gc.fresh_states(H, D, C, ams, 0x5A)
    g = _Group(x, labels, w, b, rows, keep, st, B)
    stride, content, single, work = hf.group_state_stride(D, C, ams), gc.content_bytes(D, C, ams), hf.state_bytes(D, C, ams), hf.workspace_bytes(B, D, C)
    # the single steps' operands: clones of head h's slices, each its own allocation
    ones = [dict(w=g.w[h].clone(), b=g.b[h].clone(), rows=g.rows[h].clone(), keep=None if keep is None else g.keep[h].clone(),
                 st=torch.zeros((single,), dtype=torch.uint8, device=DEV), ws=torch.empty((work,), dtype=torch.uint8, device=DEV)) for h in range(H)]
    wt, bt, stt = w.copy(), b.copy(), st.copy()                      # the host twin's, carried from step to step
    for s in range(gc.STEPS):
        table = gc.hyper(H, var["keep"], s)
        g.step(table, clear=s == 0, **_flags(var))
        for h, o in enumerate(ones):
            hf.step(g.x, g.labels, o["w"], o["b"], o["st"], o["ws"], o["rows"], o["keep"], float(table[h, 6]), **gc.single_kw(table, h, var, clear=s == 0))
        gw, gb, gst, gws = g.host()
        for h, o in enumerate(ones):
            what = "%s step %d head %d" % (gc.case_id(case), s, h)
            got, want = hf.workspace_views(gws[h * work: (h + 1) * work], B, C), hf.workspace_views(o["ws"].cpu().numpy(), B, C)
            for name in ("row_src", "z", "g", "row_loss"):
                _same(got[name], want[name], what + ": " + name)
            _same(gw[h], o["w"], what + ": w")
            _same(gb[h], o["b"], what + ": b")
            _same(gst[h * stride: h * stride + content], o["st"].cpu().numpy()[:content], what + ": state")
            assert (gst[h * stride + content: (h + 1) * stride] == 0x5A).all(), what + ": padding bytes of the state written"
        # the group twin on the device's own z, g and row losses: weights, moments and figures word for word
        hf.group_step_host(x, labels, rows, table, wt, bt, stt, gws.copy(), keep, clear=s == 0, given_g=True, **_flags(var))
        _same(gw, wt, "%s step %d: w against the twin" % (gc.case_id(case), s))
        _same(gb, bt, "%s step %d: b against the twin" % (gc.case_id(case), s))
        _same(gst, stt, "%s step %d: state against the twin" % (gc.case_id(case), s))
    for h in range(H):
        words = gst[h * stride: h * stride + 40].view(np.uint64)
        assert int(words[0]) == (0 if h == var["dead"] else gc.STEPS) and int(words[2]) == gc.STEPS * int(words[1]), (h, words.tolist())


def test_a_single_step_on_a_view_continues_the_heads_fit():
    """`HeadGroup.head(h)`: views of the group's memory - two grouped steps = one grouped step and one single step on each view."""
    H, B, D, C = 3, 20, 40, 7
    x, labels, w, b, rows, _ = gc.problem(31, H, B, D, C, False)
    kw = dict(lr=[1e-2, 2e-2, 3e-2], weight_decay=[0.0, 1e-2, 1e-3], label_smoothing=[0.0, 0.1, 0.0])
    xd, ld, rd = _to(x), _to(labels), _to(rows)
    groups = []
    for _ in range(2):
        gr = hf.HeadGroup(H, D, C, DEV, amsgrad=True)
        gr.weight.copy_(_to(w))
        gr.bias.copy_(_to(b))
        groups.append(gr)
    groups[0].step(xd, ld, rd, **kw).step(xd, ld, rd, **kw)
    groups[1].step(xd, ld, rd, **kw)
    for h in range(H):
        groups[1].head(h).step(xd, ld, rd[h].contiguous(), lr=kw["lr"][h], weight_decay=kw["weight_decay"][h], label_smoothing=kw["label_smoothing"][h])
    for name in ("weight", "bias", "state"):
        _same(getattr(groups[0], name), getattr(groups[1], name), "two grouped steps against one and a single step on each view: " + name)
    figs = groups[1].epoch_figures()
    assert [f["t"] for f in figs] == [2] * H and all(f["rows"] > 0 and f["rows"] % 2 == 0 for f in figs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 9., 10. isolation, the all-declined head, determinism
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_nan_in_one_head_stays_in_that_head():
    """Head 1 gets a NaN weight and a NaN feature in a row of the cache that only it reads: every bit of heads 0 and 2 - weights,
    state, workspace - equals the run without them."""
    H, B, D, C = 3, 33, 65, 33
    var = {"keep": True, "decoupled": False, "amsgrad": True, "dead": None}
    _, _, w, b, _, keep = gc.problem(41, H, B, D, C, True, declined=False)
    rng = np.random.default_rng(4)
    x = (rng.integers(-64, 65, (3 * B, D)) / 64.0).astype(F32)
    labels = rng.integers(0, C, 3 * B).astype(np.int32)
    rows = np.stack([np.arange(h * B, (h + 1) * B) for h in range(H)]).astype(np.int32)        # disjoint rows per head
    bad_x, bad_w = x.copy(), w.copy()
    bad_x[B + 3, 5] = np.nan
    bad_w[1, 2, 7] = np.nan
    results = []
    for xx, ww in ((x, w), (bad_x, bad_w)):
        g = _Group(xx, labels, ww, b, rows, keep, gc.fresh_states(H, D, C, True), B)
        for s in range(2):
            g.step(gc.hyper(H, True, s), clear=s == 0, **_flags(var))
        results.append(g.host())
    stride, work = hf.group_state_stride(D, C, True), hf.workspace_bytes(B, D, C)
    (w0, b0, s0, k0), (w1, b1, s1, k1) = results
    for h in (0, 2):
        _same(w0[h], w1[h], "head %d: w" % h)
        _same(b0[h], b1[h], "head %d: b" % h)
        _same(s0[h * stride: (h + 1) * stride], s1[h * stride: (h + 1) * stride], "head %d: state" % h)
        _same(k0[h * work: (h + 1) * work], k1[h * work: (h + 1) * work], "head %d: workspace" % h)
    assert np.isnan(w1[1]).any() and not np.isnan(w1[[0, 2]]).any()
    v = hf.workspace_views(k1[work: 2 * work], B, C)
    assert v["row_src"][3] == -1 and (np.delete(v["row_src"], 3) >= 0).all()          # the NaN feature declined its row, and only it


def test_an_all_declined_head_between_live_heads_and_determinism():
    H, B, D, C = 3, 40, 70, 9
    case = (H, B, D, C, {"keep": True, "decoupled": True, "amsgrad": False, "dead": 1})
    x, labels, w, b, rows, keep = gc.problem(51, H, B, D, C, True, 1)
    one, two = _run_group(case, 51, 2, fill=0xFF), _run_group(case, 51, 2, fill=0xFF)
    for a, c, name in zip(one, two, ("w", "b", "state", "workspace")):
        _same(a, c, "the same two steps twice: " + name)
    gw, gb, gst, gws = one
    stride, content = hf.group_state_stride(D, C, False), gc.content_bytes(D, C, False)
    _same(gw[1], w[1], "the all-declined head: w")
    _same(gb[1], b[1], "the all-declined head: b")
    assert not gst[stride: stride + content].any(), "the all-declined head: t, figures or moments written"
    v = hf.workspace_views(gws[hf.workspace_bytes(B, D, C): 2 * hf.workspace_bytes(B, D, C)], B, C)
    assert (v["row_src"] == -1).all() and np.isnan(v["row_loss"]).all() and not v["g"].any() and not v["z"].any()
    for h in (0, 2):
        words = gst[h * stride: h * stride + 40].view(np.uint64)
        assert int(words[0]) == 2 and int(words[1]) >= 1 and not np.array_equal(gw[h], w[h])


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. guard bands
# ---------------------------------------------------------------------------------------------------------------------------------
def test_group_guard_bands_at_element_alignment():
    """The two-fills rule of `guard` with every buffer at its element alignment (fp32 / int32 / the hyper table 4, keep 1, the states
    8, the workspaces 4: aligned to that and not to twice that), the states exactly `group_state_bytes` and the workspaces exactly
    `group_workspace_bytes`, under fills 0xFF and 0x5A: the bands and the read-only operands (the hyper table among them) stay
    untouched, and w, b, state and workspace are identical under both fills and equal to the unguarded call.  A wrong stride shows
    here: H = 3 heads of an AMSGrad state whose content is no multiple of 8."""
    H = 3
    for (B, D, C) in ((45, 70, 35), (5, 2, 1)):        # (5, 2, 1): the content of a state is 100 bytes, the stride 104
        var = {"keep": True, "decoupled": False, "amsgrad": True, "dead": None}
        case = (H, B, D, C, var)
        x, labels, w, b, rows, keep = gc.problem(61, H, B, D, C, True, declined=B >= 6)
        table = gc.hyper(H, True)
        ref = _run_group(case, 61, 1, table_of=lambda s: table)
        need = {"state": 8, "workspace": 4, "w": 4, "b": 4}
        results = []
        for fill in guard.FILLS:
            g = guard.Guard(fill, device=DEV, shift=guard.min_placement(lambda dtype, kind, who: need.get(who, 1 if dtype == torch.uint8 else 4)))
            xd, ld, rd, kd, hd = (g.place(torch.from_numpy(t)) for t in (x, labels, rows, keep, table))
            wd, bd = g.empty(w.shape, torch.float32, "w"), g.empty(b.shape, torch.float32, "b")
            sd = g.empty((hf.group_state_bytes(H, D, C, True),), torch.uint8, "state")
            wsd = g.empty((hf.group_workspace_bytes(H, B, D, C),), torch.uint8, "workspace")
            assert sd.data_ptr() % 16 == 8 and wsd.data_ptr() % 8 == 4 and wd.data_ptr() % 8 == 4 and kd.data_ptr() % 2 == 1 and hd.data_ptr() % 8 == 4
            wd.copy_(torch.from_numpy(w))
            bd.copy_(torch.from_numpy(b))
            sd.copy_(torch.from_numpy(gc.fresh_states(H, D, C, True)))
            hf.group_step(xd, ld, rd, hd, wd, bd, sd, wsd, kd, clear=True, **_flags(var))
            g.check()
            results.append((wd.cpu().numpy(), bd.cpu().numpy(), sd.cpu().numpy(), wsd.cpu().numpy()))
        for k, name in enumerate(("w", "b", "state", "workspace")):
            _same(results[0][k], results[1][k], "B=%d D=%d C=%d fill 0xFF against fill 0x5A: %s" % (B, D, C, name))
            _same(results[0][k], ref[k], "B=%d D=%d C=%d guarded against unguarded: %s" % (B, D, C, name))


# ---------------------------------------------------------------------------------------------------------------------------------
# 12. graph replay and late operands
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_group_step_replays_with_the_table_of_replay_time():
    """A captured grouped step replayed twice, the `lr` column of the hyper table rewritten on the stream between the replays =
    two eager steps with those two tables: the table is read on the device, t lives in the state, and the clearing kernel replays
    (a stale n would double the gradient's divisor)."""
    H, B, D, C = 3, 64, 128, 18
    var = {"keep": True, "decoupled": False, "amsgrad": False, "dead": None}
    case = (H, B, D, C, var)
    x, labels, w, b, rows, keep = gc.problem(71, H, B, D, C, True)
    tables = [gc.hyper(H, True, 0), gc.hyper(H, True, 0)]
    tables[1][:, 0] *= F32(3.0)
    eager = _run_group(case, 71, 2, table_of=lambda s: tables[s])
    # (the eager run clears with its first step; so does the graph's first replay below: fresh states make `clear` a no-op)
    g = _Group(x, labels, w, b, rows, keep, gc.fresh_states(H, D, C, False), B)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    t0, t1 = _to(tables[0]), _to(tables[1])
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            hf.group_step(g.x, g.labels, g.rows, g.hyper, g.w, g.b, g.st, g.ws, g.keep, **_flags(var))
        g.w.copy_(torch.from_numpy(w))                 # (capture does not run the step; start from the same weights anyway)
        g.b.copy_(torch.from_numpy(b))
        g.st.zero_()
        g.hyper.copy_(t0)
        graph.replay()
        g.hyper[:, 0].copy_(t1[:, 0])                  # the lr column only, on the stream, between the replays
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    for a, c, name in zip(eager, g.host(), ("w", "b", "state", "workspace")):
        _same(a, c, "two replays against two eager steps: " + name)
    one_table = _run_group(case, 71, 2, table_of=lambda s: tables[0])
    assert not np.array_equal(one_table[0], eager[0]), "the second table changes nothing: the test cannot see where it is read"


def _group_run():
    """The closure of the stream rules (`stream_cases`): w, b and the states are written in place, so each is a copy of its placed
    operand made on the call's own stream."""
    H, B, D, C = 3, 45, 70, 35
    var = {"keep": True, "decoupled": True, "amsgrad": True, "dead": None}
    x, labels, w, b, rows, keep = gc.problem(81, H, B, D, C, True)
    table, st = gc.hyper(H, True), gc.fresh_states(H, D, C, True)
    t = torch.from_numpy

    def run(place):
        xd, ld, rd, kd, hd = place(t(x)), place(t(labels)), place(t(rows)), place(t(keep)), place(t(table))
        wd, bd, sd = place(t(w)).clone(), place(t(b)).clone(), place(t(st)).clone()
        wsd = torch.empty((hf.group_workspace_bytes(H, B, D, C),), dtype=torch.uint8, device=DEV)
        hf.group_step(xd, ld, rd, hd, wd, bd, sd, wsd, kd, clear=True, **_flags(var))
        return wd, bd, sd, wsd
    return run


def test_group_step_with_late_operands_and_a_blocked_default_stream():
    """Every operand - the hyper table included - produced late on a side stream while the default stream is idle, then ready while
    the default stream is held by a delay (`stream_cases.late_rule`, delays within its `CAP_MS`)."""
    sc.late_rule(_group_run(), [hf], what="head_fit.group_step")


def test_group_step_captured_and_replayed_on_other_operands():
    sc.capture_rule(_group_run(), [hf], what="head_fit.group_step")


# ---------------------------------------------------------------------------------------------------------------------------------
# 13. flag 8 on the device
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[1] == 33], ids=[gc.case_id(c) for c in CASES if c[1] == 33])
def test_evaluate_only_on_the_device(case):
    H, B, D, C, var = case
    ams = var["amsgrad"]
    x, labels, w, b, rows, _ = gc.problem(91, H, B, D, C, False, var["dead"])
    table = gc.hyper(H, False)
    stride = hf.group_state_stride(D, C, ams)
    g = _Group(x, labels, w, b, rows, None, gc.fresh_states(H, D, C, ams, 0x5A), B)
    g.step(table, clear=True, **_flags(var))                         # one training step: t = 1, moments set
    w1, b1, st1, _ = g.host()
    g.step(table, evaluate=True, **_flags(var))
    we, be, ste, wse = g.host()
    _same(we, w1, "evaluate: w")
    _same(be, b1, "evaluate: b")
    # the twin's evaluate on the device's own z and row losses: every state word
    wt, bt, stt = w1.copy(), b1.copy(), st1.copy()
    hf.group_step_host(x, labels, rows, table, wt, bt, stt, wse.copy(), None, evaluate=True, given_g=True, **_flags(var))
    _same(ste, stt, "evaluate: state against the twin")
    # a training step on a copy adds the same figures and writes the same workspace
    c = _Group(x, labels, w1, b1, rows, None, st1, B)
    c.step(table, **_flags(var))
    _, _, stc, wsc = c.host()
    _same(wse, wsc, "evaluate: the workspace is the training step's")
    for h in range(H):
        e, o, t = (a[h * stride: h * stride + 40].view(np.uint64) for a in (ste, st1, stc))
        assert e[0] == o[0] and e[1:5].tolist() == t[1:5].tolist() and e[2] == 2 * o[2], (h, e.tolist(), o.tolist(), t.tolist())
        _same(ste[h * stride + 40: (h + 1) * stride], st1[h * stride + 40: (h + 1) * stride], "evaluate: moments and padding of head %d" % h)
    g.step(table, evaluate=True, clear=True, **_flags(var))          # flag 4 with flag 8 clears first
    once = g.host()[2]
    g.step(table, evaluate=True, **_flags(var))                      # two calls accumulate
    twice = g.host()[2]
    for h in range(H):
        a, c2 = once[h * stride: h * stride + 40].view(np.uint64), twice[h * stride: h * stride + 40].view(np.uint64)
        assert a[2] == a[1] and c2[2:5].tolist() == (2 * a[2:5]).tolist() and c2[0] == a[0]
    _same(g.host()[0], w1, "four evaluate calls: w")
    with pytest.raises(ValueError, match="keep"):
        hf.group_step(g.x, g.labels, g.rows, g.hyper, g.w, g.b, g.st, g.ws, torch.ones((H, B, D), dtype=torch.uint8, device=DEV), evaluate=True, **_flags(var))


def test_head_group_evaluate_leaves_the_weights():
    H, B, D, C = 4, 50, 32, 5
    x, labels, w, b, rows, _ = gc.problem(93, H, B, D, C, False)
    gr = hf.HeadGroup(H, D, C, DEV, generator=torch.Generator().manual_seed(2))
    xd, ld, rd = _to(x), _to(labels), _to(rows)
    gr.step(xd, ld, rd, lr=[1e-2, 2e-2, 3e-2, 4e-2], label_smoothing=0.1)
    before = (gr.weight.clone(), gr.bias.clone(), gr.state.clone())
    train = gr.epoch_figures()
    figs = gr.new_epoch().evaluate(xd, ld, rd).epoch_figures()
    assert torch.equal(gr.weight, before[0]) and torch.equal(gr.bias, before[1])
    for h in range(H):
        assert figs[h]["t"] == 1 and figs[h]["rows"] == train[h]["rows"] > 0 and 0.0 <= figs[h]["accuracy"] <= 1.0 and figs[h]["loss"] > 0
    st = gr.state.view(H, gr.stride)
    assert torch.equal(st[:, 40:], before[2].view(H, gr.stride)[:, 40:]) and torch.equal(st[:, :8], before[2].view(H, gr.stride)[:, :8])


# ---------------------------------------------------------------------------------------------------------------------------------
# 14., 15. the head index: a grid 257 deep, offsets past 2^31 elements
# ---------------------------------------------------------------------------------------------------------------------------------
def test_257_heads_against_the_twin():
    H, B, D, C = 257, 2, 3, 2
    var = {"keep": True, "decoupled": False, "amsgrad": True, "dead": 200}
    x, labels, w, b, rows, keep = gc.problem(95, H, B, D, C, True, 200)
    st = gc.fresh_states(H, D, C, True, 0x5A)
    g = _Group(x, labels, w, b, rows, keep, st, B)
    wt, bt, stt = w.copy(), b.copy(), st.copy()
    for s in range(2):
        table = gc.hyper(H, True, s)
        table[:, 6] = F32(1.25)                          # (0.75 - 0.05 h turns negative far below 257 heads)
        table[:, 1:3] = np.clip(table[:, 1:3], 0.5, 0.999)
        g.step(table, clear=s == 0, **_flags(var))
        gw, gb, gst, gws = g.host()
        hf.group_step_host(x, labels, rows, table, wt, bt, stt, gws.copy(), keep, clear=s == 0, given_g=True, **_flags(var))
        _same(gw, wt, "step %d: w" % s)
        _same(gb, bt, "step %d: b" % s)
        _same(gst, stt, "step %d: state" % s)
    stride = hf.group_state_stride(D, C, True)
    ts = [int(gst[h * stride: h * stride + 8].view(np.uint64)[0]) for h in range(H)]
    assert ts == [0 if h == 200 else 2 for h in range(H)]              # (every other head has a row left beside its padding)


def test_head_offsets_past_2_31_elements():
    """H = 3, D = 65 536, C = 16 384, B = 1: head 2's weights start at element 2^31 exactly and its state 16 GiB into the states.
    Head 2 against the single step on cloned slices, bit for bit.  The clone lives in head 0's memory (refilled with head 2's
    initial weights and a fresh state after the grouped step), so the case holds 12 GiB of weights, 24 GiB of states and one 4 GiB
    copy of head 2's initial weights: about 41 GiB; it skips, with the numbers, where the device does not have them free."""
    H, B, D, C, N = 3, 1, 65536, 16384, 4
    stride, single = hf.group_state_stride(D, C, False), hf.state_bytes(D, C, False)
    assert 2 * C * D == 2 ** 31 and stride == single
    big_cases.need_memory(H * C * D * 4 + H * stride + C * D * 4 + 2 ** 30, "head offsets past 2^31 elements")
    gen = torch.Generator(device=DEV).manual_seed(97)
    x = (torch.randint(-64, 65, (N, D), device=DEV, generator=gen) / 64.0).to(torch.float32)
    labels = torch.tensor([5, 16383, 77, 0], dtype=torch.int32, device=DEV)
    rows = torch.tensor([[0], [1], [2]], dtype=torch.int32, device=DEV)
    table = gc.hyper(H, False)
    hyper = _to(table)
    w = torch.empty((H, C, D), dtype=torch.float32, device=DEV)
    for h in range(H):
        w[h].uniform_(-1.0 / 256, 1.0 / 256, generator=gen)
    b = torch.zeros((H, C), dtype=torch.float32, device=DEV).uniform_(-0.1, 0.1, generator=gen)
    w2, b2 = w[2].clone(), b[2].clone()
    state = torch.zeros((H * stride,), dtype=torch.uint8, device=DEV)
    ws = torch.empty((hf.group_workspace_bytes(H, B, D, C),), dtype=torch.uint8, device=DEV)
    var = {"decoupled": False, "amsgrad": False}
    try:
        hf.group_step(x, labels, rows, hyper, w, b, state, ws, None, clear=True, **var)
        torch.cuda.synchronize()
        heads = state.view(H, stride)[:, :40].cpu().numpy().view(np.uint64)
        assert heads[:, 0].tolist() == [1, 1, 1] and heads[:, 1].tolist() == [1, 1, 1], heads.tolist()
        assert not torch.equal(w[2, :64], w2[:64])                          # head 2 moved
        # the single step on clones of head 2's slices, in head 0's memory
        w[0].copy_(w2)
        b0 = b2.clone()
        s0 = state[:single]
        s0.zero_()
        ws0 = torch.empty((hf.workspace_bytes(B, D, C),), dtype=torch.uint8, device=DEV)
        hf.step(x, labels, w[0], b0, s0, ws0, rows[2].clone(), None, 1.0, **gc.single_kw(table, 2, var, clear=True))
        torch.cuda.synchronize()
        assert torch.equal(b0.view(torch.int32), b[2].view(torch.int32)), "b of head 2"
        work = hf.workspace_bytes(B, D, C)
        assert torch.equal(ws0, ws[2 * work: 3 * work]), "workspace of head 2"
        for c0 in range(0, C, 1024):
            assert torch.equal(w[0, c0: c0 + 1024].view(torch.int32), w[2, c0: c0 + 1024].view(torch.int32)), "w of head 2, classes from %d" % c0
        s2 = state[2 * stride: 2 * stride + single]
        for at in range(0, single, 2 ** 28):
            assert torch.equal(s0[at: at + 2 ** 28], s2[at: at + 2 ** 28]), "state of head 2, bytes from %d" % at
        print("head offsets past 2^31 elements: head 2's w at element %d, its state at byte %d; peak device memory %.1f GiB" % (
            2 * C * D, 2 * stride, torch.cuda.max_memory_allocated() / 2 ** 30))
    finally:
        del w, w2, state, ws
        big_cases.release()


# ---------------------------------------------------------------------------------------------------------------------------------
# 16. end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _separable(N=600, D=64, C=6, seed=3):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((C, D)) * 0.6
    labels = rng.integers(0, C, N).astype(np.int32)
    feats = (centers[labels] + rng.standard_normal((N, D))).astype(F32)
    return _to(feats), _to(labels)


def _generators(seed):
    """A CPU generator and the device generator `fit_head`'s convention derives from it (the draw comes before the heads')."""
    cpu = torch.Generator().manual_seed(seed)
    dev = torch.Generator(device=DEV)
    dev.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=cpu).item()))
    return cpu, dev


def _figures_on_a_copy(head, feats, labels, rows_all, B, label_smoothing):
    """Validation figures of a `LinearHead` without touching it: steps at lr = 0 on a copy (its weights do not move)."""
    c = hf.LinearHead.__new__(hf.LinearHead)
    c.D, c.C, c.amsgrad, c.device = head.D, head.C, head.amsgrad, head.device
    c.weight, c.bias, c.state, c._workspaces, c._clear = head.weight.clone(), head.bias.clone(), head.state.clone(), {}, True
    for lo in range(0, rows_all.shape[0], B):
        c.step(feats, labels, rows_all[lo: lo + B].contiguous(), lr=0.0, label_smoothing=label_smoothing)
    assert torch.equal(c.weight, head.weight)
    return c.epoch_figures()


def test_cross_validate_equals_five_single_fits():
    feats, labels = _separable()
    N, D, C, B, H, epochs = 600, 64, 6, 32, 5, 3
    kw = dict(lr=5e-3, weight_decay=1e-4, label_smoothing=0.05)
    res = hf.cross_validate(feats, labels, n_folds=H, epochs=epochs, batch_size=B, seed=42, dropout=0.1, num_classes=C,
                            generator=torch.Generator().manual_seed(9), **kw)
    assert {"n_folds", "fold_results", "mean_accuracy", "std_accuracy", "history"} <= set(res) and res["n_folds"] == H
    assert [r["fold"] for r in res["fold_results"]] == [1, 2, 3, 4, 5] and all(set(r) == {"fold", "best_validation_accuracy"} for r in res["fold_results"])
    acc = [r["best_validation_accuracy"] for r in res["fold_results"]]
    assert res["mean_accuracy"] == float(np.mean(acc)) and res["std_accuracy"] == float(np.std(acc))
    # five single fits on the same rows, the same permutations and the same masks
    cpu, dev = _generators(9)
    heads = [hf.LinearHead(D, C, DEV, generator=cpu) for _ in range(H)]
    folds = hf.kfold_rows(N, H, 42)
    train = [_to(tr) for tr, _ in folds]
    val_rows = hf.padded_rows([_to(va) for _, va in folds], B, DEV)
    best = [0.0] * H
    for e in range(epochs):
        rows_all = hf.epoch_rows(train, B, dev)
        for head in heads:
            head.new_epoch()
        for lo in range(0, rows_all.shape[1], B):
            keep = hf.draw_keep(H, B, D, 0.1, DEV, dev)
            for h, head in enumerate(heads):
                head.step(feats, labels, rows_all[h, lo: lo + B].contiguous(), keep[h].contiguous(), dropout=0.1, **kw)
        for h, head in enumerate(heads):
            fig, vfig = head.epoch_figures(), _figures_on_a_copy(head, feats, labels, val_rows[h], B, kw["label_smoothing"])
            hist = res["history"][h]
            assert (hist["train_acc"][e], hist["train_loss"][e]) == (fig["accuracy"], fig["loss"]), (h, e)
            assert (hist["val_acc"][e], hist["val_loss"][e]) == (vfig["accuracy"], vfig["loss"]) and vfig["rows"] == len(folds[h][1]), (h, e)
            best[h] = max(best[h], vfig["accuracy"])
    group = res["group"]
    for h, head in enumerate(heads):
        _same(group.weight[h], head.weight, "fold %d: weights" % h)
        _same(group.bias[h], head.bias, "fold %d: bias" % h)
        gs, hs = group.head(h).state.cpu().numpy(), head.state.cpu().numpy()      # (n and the figures are the last evaluate's in the group)
        _same(gs[:8], hs[:8], "fold %d: t" % h)
        _same(gs[40:], hs[40:], "fold %d: moments" % h)
    assert acc == best and min(acc) > 0.8, (acc, best)              # (separable by construction: the fits learn)
    # a head of the group as a classifier
    h = 3
    view = group.head(h)
    model = types.SimpleNamespace(resnet=types.SimpleNamespace(fc=torch.nn.Sequential(torch.nn.Dropout(0.1), torch.nn.Linear(D, C)).to(DEV)))
    view.load_into(model)
    assert torch.equal(model.resnet.fc[1].weight.detach(), group.weight[h]) and torch.equal(model.resnet.fc[1].bias.detach(), group.bias[h])
    z = view.logits(feats[:40].contiguous())
    _same(z, ops.linear_f32(feats[:40].contiguous(), group.weight[h].clone(), None, group.bias[h].clone()), "logits of a view against the slice")
    want = feats[:40].double() @ group.weight[h].double().T + group.bias[h].double()
    assert float((z.double() - want).abs().max()) < 1e-4 and view.as_classifier()[0].data_ptr() == group.weight[h].data_ptr()


def test_sweep_heads_ranks_like_a_loop_of_single_fits():
    feats, labels = _separable(seed=5)
    vfeats, vlabels = feats[480:].contiguous(), labels[480:].contiguous()
    feats, labels = feats[:480].contiguous(), labels[:480].contiguous()
    N, D, C, B, epochs = 480, 64, 6, 32, 2
    trials = [dict(lr=1e-4, weight_decay=0.0, dropout=0.0, label_smoothing=0.0), dict(lr=5e-3, weight_decay=1e-4, dropout=0.1, label_smoothing=0.0),
              dict(lr=2e-2, weight_decay=1e-3, dropout=0.2, label_smoothing=0.1), dict(lr=1e-3, weight_decay=1e-2, dropout=0.5, label_smoothing=0.05)]
    res = hf.sweep_heads(feats, labels, vfeats, vlabels, trials, epochs=epochs, batch_size=B, num_classes=C, generator=torch.Generator().manual_seed(13))
    H = len(trials)
    assert len(res["trials"]) == H and res["best_params"] == res["trials"][res["best_trial"]]["params"]
    cpu, dev = _generators(13)
    first = hf.LinearHead(D, C, DEV, generator=cpu)
    cache, cache_labels = torch.cat([feats, vfeats]).contiguous(), torch.cat([labels, vlabels]).contiguous()
    val_rows = hf.padded_rows([torch.arange(N, N + 120, dtype=torch.int32, device=DEV)], B, DEV)[0]
    heads = []
    for _ in range(H):
        one = hf.LinearHead(D, C, DEV)
        one.weight, one.bias = first.weight.clone(), first.bias.clone()
        heads.append(one)
    drop = [torch.tensor(t["dropout"], dtype=torch.float32, device=DEV) for t in trials]
    val = [[] for _ in range(H)]
    for e in range(epochs):
        perm = torch.randperm(N, device=DEV, generator=dev).to(torch.int32)
        rows_all = hf.padded_rows([perm], B, DEV)[0]
        for lo in range(0, rows_all.shape[0], B):
            u = torch.rand((B, D), device=DEV, generator=dev)
            for h, (head, t) in enumerate(zip(heads, trials)):
                head.step(cache, cache_labels, rows_all[lo: lo + B].contiguous(), (u >= drop[h]).to(torch.uint8), lr=t["lr"],
                          weight_decay=t["weight_decay"], dropout=t["dropout"], label_smoothing=t["label_smoothing"])
        for h, (head, t) in enumerate(zip(heads, trials)):
            val[h].append(_figures_on_a_copy(head, cache, cache_labels, val_rows, B, t["label_smoothing"]))
    for h in range(H):
        assert res["trials"][h]["val_acc"] == [f["accuracy"] for f in val[h]] and res["trials"][h]["val_loss"] == [f["loss"] for f in val[h]], h
        _same(res["group"].weight[h], heads[h].weight, "trial %d: weights" % h)
    ranked = max(range(H), key=lambda h: (max(f["accuracy"] for f in val[h]), -val[h][-1]["loss"], -h))
    assert res["best_trial"] == ranked and ranked != 0, (res["best_trial"], ranked)     # (lr 1e-4 for two epochs cannot win)
