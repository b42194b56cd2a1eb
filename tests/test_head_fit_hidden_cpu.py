"""CPU: the hidden-layer head-fitting step - a first step worked by hand, the float64 rule (`head_fit.hidden_step_rule`) against
torch over 25 steps, the host twin (`head_fit.hidden_step_host`) against the float32 rule word for word over `fit_hidden_cases`,
the twin's layer 2 against `head_fit.step_host` on (h, lab, keep2), declined rows, the C ABI of the four entry points, the refusals
of `head_fit.hidden_step` under `operand_cases`' stub (nothing launches), `HiddenHead`'s initialisation, and
tools/head_fit_hidden_check.cpp under the address and undefined-behaviour sanitizers."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fit_cases as fc
import fit_hidden_cases as hc
import operand_cases as oc
from frmap_amd import _lib, head_fit as hf, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CASES = hc.cases()


def _same(a, b, what):
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d bytes differ, first at byte %d" % (what, bad.size, int(bad[0]))


def _host_step(p, var, s, w, st, ws=None, given_g=False, clear=None):
    """Step `s` of a variation through the host twin on the weights `w` = [w1, b1, w2, b2] and the state `st`, in place."""
    k1s, k2s = hc.keep_scales(var)
    return hf.hidden_step_host(p["x"], p["labels"], *w, st, ws, p["rows"], p["keep1"], k1s, p["keep2"], k2s, given_g=given_g,
                               **hc.step_kw(var, s, clear))


def _weights(p):
    return [p[k].copy() for k in ("w1", "b1", "w2", "b2")]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. a first step by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_first_step_by_hand():
    """B = D = Hd = C = 2.  Hidden unit (1, 1) is negative (a = -3), hidden unit (0, 1) is masked.  With fresh moments the first
    Adam step moves a parameter by -lr sign(grad) (m / sqrt(v) = g / |g| after the bias corrections, eps = 1e-8 aside) and leaves a
    parameter with a zero gradient where it is."""
    x = np.array([[1.0, 2.0], [3.0, -1.0]])
    labels = np.array([0, 1])
    w1, b1 = np.array([[0.5, 0.25], [-1.0, 0.5]]), np.array([0.0, 0.5])
    w2, b2 = np.array([[0.5, 1.0], [-0.5, 2.0]]), np.array([0.0, 0.0])
    keep2 = np.array([[1, 0], [1, 1]], np.uint8)
    lr = 0.125
    r = hf.hidden_step_rule(x, labels, w1, b1, w2, b2, keep2=keep2, keep2_scale=2.0, lr=lr)
    # a = [[0.5 + 0.5, -1 + 1 + 0.5], [1.5 - 0.25, -3 - 0.5 + 0.5]]
    assert np.array_equal(r["h"], [[1.0, 0.5], [1.25, 0.0]]) and r["lab"].tolist() == [0, 1] and r["n"] == 2
    # h' = [[2, 0], [2.5, 0]];  z = h' w2^T = [[1, -1], [1.25, -1.25]]
    assert np.array_equal(r["z"], [[1.0, -1.0], [1.25, -1.25]])
    p0, p1 = 1.0 / (1.0 + math.exp(-2.0)), 1.0 / (1.0 + math.exp(-2.5))          # the probability of class 0 in rows 0 and 1
    assert abs(p0 - 0.880797) < 1e-6 and abs(p1 - 0.924142) < 1e-6
    g = np.array([[(p0 - 1.0) / 2, (1.0 - p0) / 2], [p1 / 2, -p1 / 2]])         # (p - y) / n: [[-0.059601, 0.059601], [0.462071, -0.462071]]
    assert np.allclose(r["g"], g, atol=1e-15) and np.allclose(r["g"], [[-0.059601, 0.059601], [0.462071, -0.462071]], atol=1e-6)
    assert np.allclose(r["row_loss"], [-math.log(p0), -math.log(1.0 - p1)], atol=1e-15)
    assert np.allclose(r["row_loss"], [0.126928, 2.578890], atol=1e-6) and abs(r["loss"] - (0.126928 + 2.578890) / 2) < 1e-6
    # s = g w2 = [[0.5 g00 - 0.5 g01, g00 + 2 g01], ...] = [[g00, g01], [g10, g11]] here;  da = gate * s * 2
    da = np.array([[2 * g[0, 0], 0.0], [2 * g[1, 0], 0.0]])                     # (0, 1) masked, (1, 1) negative
    assert np.allclose(r["da"], da, atol=1e-15) and np.allclose(r["da"], [[-0.119203, 0.0], [0.924142, 0.0]], atol=1e-6)
    assert r["da"][0, 1] == 0 and r["da"][1, 1] == 0
    # dw1 = da^T x, db1 = sum_i da;  dw2 = g^T h', db2 = sum_i g
    assert np.allclose(r["dw1"], [[da[0, 0] * 1 + da[1, 0] * 3, da[0, 0] * 2 - da[1, 0]], [0.0, 0.0]], atol=1e-15)
    assert np.allclose(r["dw1"], [[2.653223, -1.162548], [0.0, 0.0]], atol=1e-6) and np.allclose(r["db1"], [0.804939, 0.0], atol=1e-6)
    assert np.allclose(r["dw2"], [[1.035975, 0.0], [-1.035975, 0.0]], atol=1e-6) and np.allclose(r["db2"], [0.402470, -0.402470], atol=1e-6)
    # the update: -lr sign(grad), nothing where the gradient is zero
    assert np.allclose(r["w1"], [[0.5 - lr, 0.25 + lr], [-1.0, 0.5]], atol=1e-7) and np.array_equal(r["w1"][1], w1[1])
    assert np.allclose(r["b1"], [0.0 - lr, 0.5], atol=1e-7) and r["b1"][1] == 0.5
    assert np.allclose(r["w2"], [[0.5 - lr, 1.0], [-0.5 + lr, 2.0]], atol=1e-7) and np.array_equal(r["w2"][:, 1], w2[:, 1])
    assert np.allclose(r["b2"], [-lr, lr], atol=1e-7)
    st = r["state"]
    assert st["layer1"]["t"] == st["layer2"]["t"] == 1 and st["layer1"]["n"] == st["layer2"]["n"] == 2
    assert st["layer2"]["rows"] == 2 and st["layer2"]["correct"] == 1 and st["layer1"]["rows"] == st["layer1"]["correct"] == st["layer1"]["loss_q"] == 0
    # the float32 rule and the twin give the same step
    f = hf.hidden_step_rule(x, labels, w1, b1, w2, b2, keep2=keep2, keep2_scale=2.0, lr=lr, dtype=F32)
    for k in ("h", "z", "da", "w1", "b1", "w2", "b2"):
        assert f[k].dtype == F32 and np.allclose(f[k], r[k], atol=1e-6), k
    w = [a.astype(F32) for a in (w1, b1, w2, b2)]
    ws = hf.hidden_step_host(x, labels, *w, np.zeros(hf.hidden_state_bytes(2, 2, 2), np.uint8), None, None, None, 1.0, keep2, 2.0, lr=lr)
    v = hf.hidden_workspace_views(ws, 2, 2, 2)
    _same(v["h"], f["h"], "h")
    _same(v["da"], f["da"], "da")
    assert np.allclose(w[0], r["w1"], atol=1e-6) and v["lab"].tolist() == [0, 1] and v["row_src1"].tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the float64 rule against torch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,decoupled,amsgrad,ls", [((7, 5, 6, 3), False, False, 0.0), ((31, 3, 33, 2), True, True, 0.1),
                                                        ((32, 64, 32, 18), False, True, 0.1), ((33, 65, 65, 33), True, False, 0.0)])
def test_float64_rule_against_torch(shape, decoupled, amsgrad, ls):
    """25 steps of Linear -> relu -> mask multiply -> Linear + F.cross_entropy(label_smoothing=) + one Adam / AdamW over the four
    parameters, float64 on both sides, fresh masks and a new learning rate every step: loss, h and all four parameters to 1e-12 (the
    bound `test_head_fit_cpu.py` holds the linear rule to; its worst measured was 7e-15)."""
    B, D, Hd, C = shape
    var = dict(hc.VARIATIONS[0], keep1=True, keep2=True)
    p = hc.problem(300 + B, B, D, Hd, C, var, declined=False)
    rng = np.random.default_rng(B)
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    lin1, lin2 = torch.nn.Linear(D, Hd).double(), torch.nn.Linear(Hd, C).double()
    with torch.no_grad():
        for dst, src in ((lin1.weight, "w1"), (lin1.bias, "b1"), (lin2.weight, "w2"), (lin2.bias, "b2")):
            dst.copy_(t(p[src]))
    params = list(lin1.parameters()) + list(lin2.parameters())
    wd = 1e-2
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(params, lr=1e-3, weight_decay=wd, amsgrad=amsgrad)
    w = [p[k].astype(np.float64) for k in ("w1", "b1", "w2", "b2")]
    st, worst = None, 0.0
    xb, yb = t(p["x"][p["rows"]]), torch.tensor(p["labels"][p["rows"]].astype(np.int64))
    for s in range(25):
        lr = 1e-2 * (1 + s % 3)
        keep1, keep2 = (rng.random((B, D)) >= 0.25).astype(np.uint8), (rng.random((B, Hd)) >= 0.5).astype(np.uint8)
        for gr in opt.param_groups:
            gr["lr"] = lr
        opt.zero_grad()
        h = torch.relu(lin1(xb * t(keep1) * (1.0 / 0.75)))
        loss = torch.nn.functional.cross_entropy(lin2(h * t(keep2) * 2.0), yb, label_smoothing=ls)
        loss.backward()
        opt.step()
        r = hf.hidden_step_rule(p["x"], p["labels"], *w, st, p["rows"], keep1, 1.0 / 0.75, keep2, 2.0, lr=lr, weight_decay=wd,
                                label_smoothing=ls, decoupled=decoupled, amsgrad=amsgrad)
        w, st = [r[k] for k in ("w1", "b1", "w2", "b2")], r["state"]
        errs = [abs(r["loss"] - float(loss.detach())), float(np.abs(r["h"] - h.detach().numpy()).max())]
        errs += [float(np.abs(a - q.detach().numpy()).max()) for a, q in zip(w, params)]
        worst = max(worst, *errs)
        assert max(errs) <= 1e-12, (shape, s, errs)
    share = float((r["h"] > 0).mean())
    print("hidden rule against torch %s: worst difference over 25 steps %.3g, share(h > 0) at the end %.2f" % (shape, worst, share))
    assert st["layer2"]["t"] == 25 and st["layer1"]["t"] == 25


# ---------------------------------------------------------------------------------------------------------------------------------
# 3., 4. the twin against the float32 rule, and its layer 2 against the single twin
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + [((33, 65, 65, 33), hc.NO_MASKS)], ids=[hc.case_id(c) for c in CASES] + ["B33-D65-Hd65-C33-no-masks"])
def test_twin_equals_the_float32_rule_word_for_word(case):
    """h, lab, row_src1, z, da, both weights, both biases and every state word bit for bit at each of three steps; g and the row loss
    within one float32 unit in the last place of their float64 values on both sides, and everything downstream on the twin's own g
    (as `test_head_fit_cpu.py` holds them).  Layer 2 of the twin is `step_host` on (h, lab, keep2), bit for bit."""
    (B, D, Hd, C), var = case
    p = hc.problem(500 + (CASES.index(case) if case in CASES else len(CASES)), B, D, Hd, C, var)
    ams = var["amsgrad"]
    k1s, k2s = hc.keep_scales(var)
    w = _weights(p)
    st = np.zeros(hf.hidden_state_bytes(D, Hd, C, ams), np.uint8)
    rw, rst = _weights(p), None
    n1 = hf.state_bytes(D, Hd, ams)
    for s in range(hc.STEPS):
        what = "%s step %d" % (hc.case_id(case), s)
        w2_before, b2_before, st2_before = w[2].copy(), w[3].copy(), st[n1:].copy()
        ws = _host_step(p, var, s, w, st)
        tw = hf.hidden_workspace_views(ws, B, Hd, C)
        kw = hc.step_kw(var, s)
        own = hf.hidden_step_rule(p["x"], p["labels"], *rw, rst, p["rows"], p["keep1"], k1s, p["keep2"], k2s, dtype=F32, **kw)
        for name in ("h", "z"):
            _same(own[name], tw[name], what + ": " + name)
        assert np.array_equal(own["lab"], tw["lab"]) and np.array_equal(own["row_src1"], tw["row_src1"]), what
        assert np.array_equal(own["row_src"], tw["row_src"]), what
        ok = tw["row_src"] >= 0
        n = int(ok.sum())
        if n:
            g64, l64 = fc.softmax64(tw["z"][ok], tw["lab"][ok], n, var["label_smoothing"], C)
            for got in (tw, own):
                assert (np.abs(got["g"][ok] - g64) <= fc.ulp32(g64)).all(), what
                assert (np.abs(got["row_loss"][ok] - l64) <= fc.ulp32(l64)).all(), what
        r = hf.hidden_step_rule(p["x"], p["labels"], *rw, rst, p["rows"], p["keep1"], k1s, p["keep2"], k2s, dtype=F32,
                                given={k: tw[k] for k in ("z", "g", "row_loss")}, **kw)
        _same(r["da"], tw["da"], what + ": da")
        for k, name in enumerate(("w1", "b1", "w2", "b2")):
            _same(r[name], w[k], what + ": " + name)
        sv = hf.hidden_state_views(st, D, Hd, C, ams)
        for layer in ("layer1", "layer2"):
            for name in sv[layer]:
                if sv[layer][name].shape:
                    _same(r["state"][layer][name], sv[layer][name], "%s: %s.%s" % (what, layer, name))
                else:
                    assert int(sv[layer][name]) == r["state"][layer][name], (what, layer, name)
        rw, rst = [r[k] for k in ("w1", "b1", "w2", "b2")], r["state"]
        # layer 2 alone: the single twin on the hidden activations
        ws2 = hf.step_host(tw["h"].copy(), tw["lab"].copy(), w2_before, b2_before, st2_before, None, None, p["keep2"], k2s, batch=B, **kw)
        _same(w2_before, w[2], what + ": w2 against the single twin")
        _same(b2_before, w[3], what + ": b2 against the single twin")
        _same(st2_before, st[n1:], what + ": the second part of the state against the single twin")
        _same(ws2, ws[8 * B * Hd + 8 * B:], what + ": the tail of the workspace against the single twin")
    head1, head2 = st[:64].view(np.uint64), st[n1: n1 + 64].view(np.uint64)
    assert head1[0] == head2[0] == hc.STEPS and head1[1] == head2[1] >= 1 and not head1[2:].any() and head2[2] == hc.STEPS * head2[1]
    if p["bad"]:
        assert (tw["row_src1"][p["bad"]] == -1).all() and (tw["lab"][p["bad"]] == -1).all() and int(head2[1]) == B - 3
        assert not tw["h"][p["bad"]].any() and not tw["da"][p["bad"]].any()
    assert not np.array_equal(w[0], p["w1"]) and not np.array_equal(w[2], p["w2"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. declined rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", hc.VARIATIONS, ids=[v["name"] for v in hc.VARIATIONS])
def test_bad_rows_count_for_nothing(var):
    """The step with the three bad rows equals the step on the batch without them (B smaller: the same n), in every parameter and
    moment bit.  B <= 128, so that every sum over the batch is one chain on both sides: a declined row adds fmaf(+0, +0, c) = c."""
    B, D, Hd, C = 33, 65, 65, 33
    p = hc.problem(41, B, D, Hd, C, var)
    q = hc.without_bad_rows(p)
    assert len(p["bad"]) == 3 and q["B"] == B - 3
    wp, wq = _weights(p), _weights(q)
    sp, sq = (np.zeros(hf.hidden_state_bytes(D, Hd, C, var["amsgrad"]), np.uint8) for _ in range(2))
    for s in range(hc.STEPS):
        _host_step(p, var, s, wp, sp)
        _host_step(q, var, s, wq, sq)
        for a, b, name in zip(wp, wq, ("w1", "b1", "w2", "b2")):
            _same(a, b, "step %d: %s" % (s, name))
        _same(sp, sq, "step %d: the state" % s)
    assert int(sp[8:16].view(np.uint64)[0]) == B - 3


def test_an_all_declined_batch_changes_nothing_but_the_workspace():
    B, D, Hd, C = 5, 4, 6, 3
    var = hc.VARIATIONS[1]
    p = hc.problem(43, B, D, Hd, C, var, declined=False)
    w = _weights(p)
    st = np.zeros(hf.hidden_state_bytes(D, Hd, C, True), np.uint8)
    _host_step(p, var, 0, w, st)
    before_w, before_st = [a.copy() for a in w], st.copy()
    dead = dict(p, rows=np.array([-1, p["N"], -7, 2 ** 31 - 1, -1], np.int32))
    ws = _host_step(dead, var, 1, w, st, np.full(hf.hidden_workspace_bytes(B, D, Hd, C), 0x5A, np.uint8), clear=False)
    for a, b in zip(w, before_w):
        _same(a, b, "a weight moved")
    n1 = hf.state_bytes(D, Hd, True)
    assert st[:8].view(np.uint64)[0] == 1 and st[n1: n1 + 8].view(np.uint64)[0] == 1, "t moved"
    assert st[8:16].view(np.uint64)[0] == 0 and st[n1 + 8: n1 + 16].view(np.uint64)[0] == 0, "n of the step is 0"
    changed = np.flatnonzero(st != before_st)
    assert set(changed.tolist()) <= set(range(8, 16)) | set(range(n1 + 8, n1 + 16)), "more than n changed in the state"
    v = hf.hidden_workspace_views(ws, B, Hd, C)
    assert (v["lab"] == -1).all() and (v["row_src1"] == -1).all() and (v["row_src"] == -1).all() and not v["h"].any() and not v["da"].any()
    assert not v["g"].any() and np.isnan(v["row_loss"]).all()
    # a NaN in w1 reaches every h row: layer 2 declines them all
    w[0][0, 0] = np.nan
    before_w = [a.copy() for a in w]
    ws = _host_step(p, var, 2, w, st, clear=False)
    v = hf.hidden_workspace_views(ws, B, Hd, C)
    assert (v["row_src1"] >= 0).all() and (v["row_src"] == -1).all() and np.isnan(v["h"][:, 0]).all() and not v["da"].any()
    for a, b in zip(w, before_w):
        _same(a, b, "a NaN in w1: a weight moved")
    assert st[:8].view(np.uint64)[0] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hidden_entry_points_are_declared_bound_and_element_aligned():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_head_fit_hidden_state_bytes", 4), ("frmap_head_fit_hidden_workspace_bytes", 4),
                       ("frmap_head_fit_hidden_step", 26), ("frmap_head_fit_hidden_step_host", 26)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10          # only symbols are added
    rows = _lib.ALIGNMENT["frmap_head_fit_hidden_step"]
    assert list(rows) == ["x", "labels", "rows", "keep1", "keep2", "w1", "b1", "w2", "b2", "state", "workspace"]
    assert all(cls == "element" for cls, _ in rows.values())
    assert [n for _, n in rows.values()] == [4, 4, 4, 1, 1, 4, 4, 4, 4, 8, 4]
    assert "frmap_head_fit_hidden_step_host" not in _lib.ALIGNMENT
    assert {"frmap_head_fit_hidden_state_bytes", "frmap_head_fit_hidden_workspace_bytes"} <= set(oc.pointer_free())
    assert not hasattr(ops, "head_fit_hidden_step") and oc.census()
    for name in ("hidden_state_bytes", "hidden_workspace_bytes", "hidden_step", "hidden_step_host", "hidden_step_rule", "HiddenHead"):
        assert callable(getattr(hf, name)), name


def test_hidden_sizes():
    lib = _lib.load()
    for D, Hd, C in ((1, 1, 1), (2, 3, 1), (128, 512, 18), (65, 65, 33)):
        for ams in (0, 1):
            n1, n2 = lib.frmap_head_fit_state_bytes(D, Hd, ams), lib.frmap_head_fit_state_bytes(Hd, C, ams)
            assert n1 % 8 == 0 and n2 % 8 == 0 and lib.frmap_head_fit_hidden_state_bytes(D, Hd, C, ams) == n1 + n2 == hf.hidden_state_bytes(D, Hd, C, bool(ams))
        for B in (1, 32, 65):
            want = 4 * (2 * B * Hd + 2 * B) + lib.frmap_head_fit_workspace_bytes(B, Hd, C)
            assert lib.frmap_head_fit_hidden_workspace_bytes(B, D, Hd, C) == want == hf.hidden_workspace_bytes(B, D, Hd, C)
    for bad in ((0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (65537, 1, 1, 0), (1, 65537, 1, 0), (1, 1, 65537, 0)):
        assert lib.frmap_head_fit_hidden_state_bytes(*bad) == 0, bad
        assert lib.frmap_head_fit_hidden_workspace_bytes(4, *bad[:3]) == 0, bad
    assert lib.frmap_head_fit_hidden_state_bytes(65536, 65536, 65536, 1) == 2 * lib.frmap_head_fit_state_bytes(65536, 65536, 1) > 2 ** 36
    assert lib.frmap_head_fit_hidden_workspace_bytes(0, 2, 2, 2) == 0 and lib.frmap_head_fit_hidden_workspace_bytes(2 ** 20 + 1, 2, 2, 2) == 0
    assert lib.frmap_head_fit_hidden_workspace_bytes(2 ** 20, 2, 65536, 65536) == 4 * (2 * 2 ** 36 + 2 * 2 ** 20) + 4 * (2 * 2 ** 36 + 2 * 2 ** 20)
    with pytest.raises(ValueError, match="Hd = 0"):
        hf.hidden_state_bytes(2, 0, 1)
    with pytest.raises(ValueError, match="B = 0"):
        hf.hidden_workspace_bytes(0, 2, 2, 1)


def test_twin_and_launcher_refusals_name_the_argument():
    """Both come before anything is read, written or launched: host dummy pointers serve."""
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.uint8)
    p = (buf.ctypes.data + 255) // 256 * 256
    ok = dict(x=p, labels=p, rows=p, keep1=0, ks1=1.0, keep2=0, ks2=1.0, w1=p, b1=p, w2=p, b2=p, state=p, workspace=p, N=1, B=1, D=1, Hd=1,
              C=1, flags=0)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)

    def args(**kw):
        a = dict(ok, **kw)
        return [a[k] for k in ("x", "labels", "rows", "keep1", "ks1", "keep2", "ks2", "w1", "b1", "w2", "b2", "state", "workspace", "N", "B",
                               "D", "Hd", "C")] + list(hyper) + [a["flags"]]
    refused = [(dict(flags=8), "flags"), (dict(flags=16), "flags"), (dict(N=0), "N"), (dict(B=0), "B"), (dict(B=2 ** 20 + 1), "B"),
               (dict(D=0), "D"), (dict(D=65537), "D"), (dict(Hd=0), "Hd"), (dict(Hd=65537), "Hd"), (dict(C=0), "C"), (dict(C=65537), "C"),
               (dict(w1=0), "null pointer"), (dict(b2=0), "null pointer"), (dict(x=0), "null pointer"), (dict(state=0), "null pointer"),
               (dict(workspace=0), "null pointer")]
    for kw, word in refused:
        for name, fn, last in (("head_fit_hidden_step_host", lib.frmap_head_fit_hidden_step_host, 0),
                               ("head_fit_hidden_step", lib.frmap_head_fit_hidden_step, None)):
            assert fn(*args(**kw), last) == -1, (name, kw)
            msg = lib.frmap_last_error().decode()
            assert msg.startswith(name + ": ") and oc.names_operand(msg, word.split()[0]), (name, kw, msg)
    for arg, need in (("x", 4), ("labels", 4), ("rows", 4), ("w1", 4), ("b1", 4), ("w2", 4), ("b2", 4), ("state", 8), ("workspace", 4)):
        assert lib.frmap_head_fit_hidden_step(*args(**{arg: p + need // 2}), None) == -1, arg
        msg = lib.frmap_last_error().decode()
        assert msg.startswith("head_fit_hidden_step: ") and "%s must be %d-byte aligned" % (arg, need) in msg, (arg, msg)
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the wrapper's refusals under the stub
# ---------------------------------------------------------------------------------------------------------------------------------
class _Cuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: all `_dev` / `_sized` ask of an operand before the library is reached."""
    @property
    def is_cuda(self):
        return True


def _gpu(t):
    return t.as_subclass(_Cuda) if isinstance(t, torch.Tensor) else t


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: None)
    monkeypatch.setattr(hf, "_stream", lambda: 0)
    return oc.install(monkeypatch)


def _valid(amsgrad=False):
    N, B, D, Hd, C = 9, 4, 8, 6, 2
    g = torch.Generator().manual_seed(1)
    return dict(x=torch.randn((N, D), generator=g), labels=torch.zeros((N,), dtype=torch.int32), w1=torch.randn((Hd, D), generator=g),
                b1=torch.zeros((Hd,)), w2=torch.randn((C, Hd), generator=g), b2=torch.zeros((C,)),
                state=torch.zeros((hf.hidden_state_bytes(D, Hd, C, amsgrad),), dtype=torch.uint8),
                workspace=torch.zeros((hf.hidden_workspace_bytes(B, D, Hd, C),), dtype=torch.uint8),
                rows=torch.tensor([0, 3, 8, -1], dtype=torch.int32), keep1=torch.ones((B, D), dtype=torch.uint8),
                keep2=torch.ones((B, Hd), dtype=torch.uint8))


ORDER = ("x", "labels", "w1", "b1", "w2", "b2", "state", "workspace", "rows", "keep1", "keep2")
# the axes along which an operand's extent is another operand's (w1's and w2's first axes GIVE Hd and C, rows' B)
DEPENDENT = {"labels": (0,), "w1": (1,), "b1": (0,), "w2": (1,), "b2": (0,), "state": (0,), "workspace": (0,), "keep1": (0, 1), "keep2": (0, 1)}


def _call(values, **kw):
    v = [_gpu(values[k]) for k in ORDER]
    return hf.hidden_step(*v[:9], v[9], 1.0, v[10], 1.0, **kw)


def test_the_valid_hidden_call_reaches_the_library(stub):
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(_valid())
    assert e.value.entry == "frmap_head_fit_hidden_step" and e.value.args_[13:18] == (9, 4, 8, 6, 2) and e.value.args_[24] == 0
    assert len(stub.calls) == 1
    v = _valid(True)
    v["keep1"] = v["rows"] = None
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(v, amsgrad=True, clear=True, decoupled=True)
    assert e.value.args_[2] == 0 and e.value.args_[3] == 0 and e.value.args_[5] != 0 and e.value.args_[14] == 4 and e.value.args_[24] == 7


@pytest.mark.parametrize("operand", sorted(DEPENDENT))
def test_a_dependent_hidden_operand_is_refused_before_the_library(operand, stub):
    """Each dependent operand one element short, one long, of the wrong rank, of the wrong dtype, and on the CPU."""
    valid = _valid()[operand]
    cases = []
    for ax in DEPENDENT[operand]:
        n = valid.shape[ax]
        cases.append(("short-axis%d" % ax, valid.narrow(ax, 0, n - 1).contiguous(), ValueError))
        cases.append(("long-axis%d" % ax, torch.cat([valid, valid.narrow(ax, 0, 1)], dim=ax).contiguous(), ValueError))
    cases.append(("rank", valid[None].contiguous() if valid.dim() == 1 else valid.reshape(-1).contiguous(), ValueError))
    cases.append(("dtype", valid.to(oc.wrong_dtype(valid.dtype)), TypeError))
    for label, bad, exc in cases:
        values = _valid()
        values[operand] = bad
        with pytest.raises(exc) as e:
            _call(values)
        assert oc.names_operand(str(e.value), operand), (operand, label, str(e.value))
    values = _valid()
    values[operand] = values[operand].clone()
    v = [values[k] if k == operand else _gpu(values[k]) for k in ORDER]          # this one stays a CPU tensor
    with pytest.raises(RuntimeError) as e:
        hf.hidden_step(*v[:9], v[9], 1.0, v[10], 1.0)
    assert oc.names_operand(str(e.value), operand)
    assert stub.calls == []


def test_free_hidden_operands_are_refused(stub):
    for operand, bad, exc in (("x", torch.zeros((9,)), ValueError), ("x", torch.zeros((9, 8), dtype=torch.float64), TypeError),
                              ("rows", torch.zeros((2, 2), dtype=torch.int32), ValueError), ("w1", None, TypeError), ("w2", None, TypeError)):
        values = _valid()
        values[operand] = bad
        with pytest.raises(exc):
            _call(values)
    with pytest.raises(ValueError, match="state"):                    # the AMSGrad state is larger
        _call(_valid(), amsgrad=True)
    v = _valid()
    v["rows"] = v["keep1"] = v["keep2"] = None
    with pytest.raises(ValueError, match="exceed"):
        _call(v, batch=10)
    with pytest.raises(ValueError):
        hf.HiddenHead(8, 0, 3, "cpu")
    with pytest.raises(ValueError):
        hf.HiddenHead(8, 4, hf.MAX_C + 1, "cpu")
    assert stub.calls == []


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. HiddenHead
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hidden_head_initialises_as_two_consecutive_linears():
    D, Hd, C = 16, 12, 4
    head = hf.HiddenHead(D, Hd, C, "cpu", amsgrad=True, generator=torch.Generator().manual_seed(7))
    torch.manual_seed(7)
    lin1, lin2 = torch.nn.Linear(D, Hd), torch.nn.Linear(Hd, C)
    assert torch.equal(head.w1, lin1.weight.detach()) and torch.equal(head.b1, lin1.bias.detach())
    assert torch.equal(head.w2, lin2.weight.detach()) and torch.equal(head.b2, lin2.bias.detach())
    gen = torch.Generator().manual_seed(7)
    one, two = hf.LinearHead(D, Hd, "cpu", generator=gen), hf.LinearHead(Hd, C, "cpu", generator=gen)
    assert torch.equal(head.w1, one.weight) and torch.equal(head.b2, two.bias)
    assert head.state.numel() == hf.hidden_state_bytes(D, Hd, C, True) and not head.state.any()
    fig = head.epoch_figures()
    assert fig["rows"] == 0 and fig["t"] == 0 and np.isnan(fig["accuracy"])
    cls = head.classifier()
    assert isinstance(cls, hf.LinearHead) and (cls.D, cls.C) == (Hd, C) and cls.weight.data_ptr() == head.w2.data_ptr()
    assert cls.state.data_ptr() == head.state.data_ptr() + hf.state_bytes(D, Hd, True) and cls.state.numel() == hf.state_bytes(Hd, C, True)
    assert cls.as_classifier()[1].data_ptr() == head.b2.data_ptr()
    assert sorted(head.state_dict()) == ["fc1.bias", "fc1.weight", "fc2.bias", "fc2.weight"]
    # load_into: a BaselineNet of matching shapes, anything else refused by name
    import frmap_amd
    model = frmap_amd.get_model("baseline", C)
    with pytest.raises(ValueError, match="fc1"):
        head.load_into(model)                                         # fc1 is [512, 128]
    with pytest.raises(ValueError, match="ResNetTransfer"):
        head.load_into(frmap_amd.get_model("cnn", C))
    own = hf.HiddenHead(128, 512, C, "cpu", generator=torch.Generator().manual_seed(3))
    own.load_into(model)
    assert torch.equal(model.fc1.weight.detach(), own.w1) and torch.equal(model.fc2.bias.detach(), own.b2)
    with pytest.raises(ValueError, match="fc2"):
        hf.HiddenHead(128, 512, C + 1, "cpu").load_into(model)
    with pytest.raises(ValueError, match="pooled"):
        hf.cache_features(frmap_amd.get_model("cnn", C), "cnn", [], layer="pooled")
    with pytest.raises(ValueError, match="layer"):
        hf.cache_features(model, "baseline", [], layer="fc1")


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the check program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_hidden_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/head_fit_hidden_check.cpp (its own `main`, head_fit_twin.h, the two rule headers and tools/head_fit_check_common.h, nothing else) built with
    -fsanitize=address,undefined (runtimes linked statically) and run directly as a child process: it sweeps the CPU table of
    `fit_hidden_cases` with every buffer a heap block of exactly its size, and exits 0."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "head_fit_hidden_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    src_path = os.path.join(ROOT, "tools", "head_fit_hidden_check.cpp")
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc, src_path, "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.stdout.splitlines()[-2:] == ["%d cases" % len(CASES), "self check passed"], run.stdout[-500:]
    src = open(src_path).read()                                                  # the program's table is this module's
    assert "shapes[][4] = {%s}" % ", ".join("{%d, %d, %d, %d}" % s for s in hc.CPU_SHAPES) in src
