"""CPU: the pair head-fitting step - a first step worked by hand, the float64 rule (`head_fit.pair_step_rule`) against torch autograd
over 25 steps, against the reference's own ContrastiveLoss (tests/golden/contrastive_loss.json), the host twin
(`head_fit.pair_step_host`) against the float32 rule word for word over `fit_pair_cases`, bad pairs, the all-declined batch, the C ABI
of the four entry points, the refusals of `head_fit.pair_step` under `operand_cases`' stub (nothing launches), `PairHead`'s
initialisation, `draw_pairs`, the synthetic fit with the float32 rule, and tools/head_fit_pair_check.cpp under the address and
undefined-behaviour sanitizers."""
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fit_pair_cases as pc
import operand_cases as oc
from frmap_amd import _lib, head_fit as hf, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CASES = pc.cases()


def _same(a, b, what):
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
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


def _host_step(p, var, s, w, b, st, ws=None, given_g=False, clear=None):
    return hf.pair_step_host(p["x"], p["left"], p["right"], p["differ"], w, b, st, ws, p["keep"], pc.keep_scale(var), given_g=given_g,
                             **pc.step_kw(var, s, clear))


def _rule_step(p, var, s, w, b, state, dtype, clear=None, given=None):
    return hf.pair_step_rule(p["x"], p["left"], p["right"], p["differ"], w, b, state, p["keep"], pc.keep_scale(var), dtype=dtype,
                             given=given, **pc.step_kw(var, s, clear))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. a first step by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_first_step_by_hand():
    """D = E = 2, w the identity, b zero: a is x.  Rows (3, 4), (4, 3), (-3, -4) have norm 5: u0 = (.6, .8), u1 = (.8, .6), u2 = -u0.
    Pair 0 = (row 0, row 1), the same identity; pair 1 = (row 0, row 2), different, margin 2.5.  With fresh moments the first Adam step
    moves a parameter by -lr sign(grad) (eps = 1e-8 aside)."""
    x = np.array([[3.0, 4.0], [4.0, 3.0], [-3.0, -4.0]])
    w, b = np.eye(2), np.zeros(2)
    left, right, differ = [0, 0], [1, 2], [0, 1]
    lr, margin, w_same, w_diff = 0.125, 2.5, 0.8, 1.2
    r = hf.pair_step_rule(x, left, right, differ, w, b, lr=lr, margin=margin, w_same=w_same, w_diff=w_diff, accept=0.5)
    assert np.array_equal(r["a"], x[[0, 0, 1, 2]]) and r["n"] == 2 and r["row_src"].tolist() == [0, 0, 1, 2]
    e = 1e-6
    # pair 0: delta = (.6 - .8 + e, .8 - .6 + e);  d^2 = 0.08 + 2 e^2 (the +-0.2 e terms cancel)
    d0 = math.sqrt((0.6 - 0.8 + e) ** 2 + (0.8 - 0.6 + e) ** 2)
    assert abs(d0 - math.sqrt(0.08 + 2e-12)) < 1e-15 and abs(r["dist"][0] - d0) < 1e-15
    assert abs(r["pair_loss"][0] - 0.8 * d0 * d0) < 1e-15 and abs(r["pair_loss"][0] - 0.064) < 1e-11
    # pair 1: delta = (1.2 + e, 1.6 + e);  d = sqrt(4 + 5.6 e + 2 e^2) = 2 + 1.4 e + ...;  loss = 1.2 (2.5 - d)^2
    d1 = math.sqrt((1.2 + e) ** 2 + (1.6 + e) ** 2)
    assert abs(d1 - (2 + 1.4e-6)) < 1e-11 and abs(r["dist"][1] - d1) < 1e-15
    assert abs(r["pair_loss"][1] - 1.2 * (2.5 - d1) ** 2) < 1e-15 and abs(r["pair_loss"][1] - 0.3) < 1e-5
    assert abs(r["loss"] - (r["pair_loss"][0] + r["pair_loss"][1]) / 2) < 1e-15
    # figures: pair 0 is a same pair at 0.283 < 0.5: accepted, right;  pair 1 a different pair at 2 >= 0.5: rejected, right
    assert r["state"]["rows"] == 2 and r["state"]["correct"] == 2 and r["state"]["t"] == 1
    assert r["state"]["loss_q"] == sum(int(round(float(F32(l)) * 2 ** 24)) for l in r["pair_loss"])      # (of the fp32 loss)
    # ga, pair 0 left: gd = (2 w_same d0 / n) delta / d0 = 0.8 delta;  ga = (gd - u (u . gd)) / 5
    gd = [0.8 * (-0.2 + e), 0.8 * (0.2 + e)]
    ugd = 0.6 * gd[0] + 0.8 * gd[1]
    want = [(gd[0] - 0.6 * ugd) / 5, (gd[1] - 0.8 * ugd) / 5]
    assert np.abs(r["ga"][0] - want).max() < 1e-16
    # ... and its right row: -gd through v = (.8, .6)
    vgd = -(0.8 * gd[0] + 0.6 * gd[1])
    assert np.abs(r["ga"][2] - [(-gd[0] - 0.8 * vgd) / 5, (-gd[1] - 0.6 * vgd) / 5]).max() < 1e-16
    # pair 1 left: q = -2 w_diff (2.5 - d1) / n = -1.2 (2.5 - d1);  delta is all but parallel to u0 (the e aside): ga ~ 1e-7
    assert np.abs(r["ga"][1]).max() < 1e-6 and np.abs(r["ga"][3]).max() < 1e-6
    for i in range(4):
        assert abs(float(r["ga"][i] @ r["a"][i])) < 1e-15                      # the gradient of a normalised row is orthogonal to it
    dw = r["ga"].T @ x[[0, 0, 1, 2]]
    assert np.abs(r["dw"] - dw).max() < 1e-16 and np.abs(r["db"] - r["ga"].sum(axis=0)).max() < 1e-16
    # m = 0.1 g, v = 0.001 g^2 and their corrections 0.1, 0.001: the step is lr g / (|g| + eps) - lr sign(g) where |g| >> eps = 1e-8
    assert np.abs(r["w"] - (w - lr * dw / (np.abs(dw) + 1e-8))).max() < 1e-12
    assert np.abs(r["b"] - (b - lr * r["db"] / (np.abs(r["db"]) + 1e-8))).max() < 1e-12
    assert abs(r["w"][0, 1] - lr) < 1e-6 and abs(r["w"][1, 0] - lr) < 1e-6         # dw[0][1], dw[1][0] = -0.0627: up by lr


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the float64 rule against torch autograd
# ---------------------------------------------------------------------------------------------------------------------------------
def _torch_loss(a, differ, P, margin, w_same, w_diff, twice=False):
    u = F.normalize(a, p=2, dim=1)
    if twice:
        u = F.normalize(u, p=2, dim=1)                                          # the model normalises, then the loss does again
    d = torch.clamp(F.pairwise_distance(u[:P], u[P:]), min=1e-8)
    y = torch.as_tensor(differ, dtype=torch.float64)
    per = (1 - y) * d.pow(2) * w_same + y * torch.clamp(margin - d, min=0.0).pow(2) * w_diff
    return per, d


@pytest.mark.parametrize("var", pc.VARIATIONS + ({"name": "adam-nomask", "keep": False, "decoupled": False, "amsgrad": False, "weight_decay": 0.0},),
                         ids=lambda v: v["name"])
def test_float64_rule_against_torch_over_25_steps(var):
    P, D, E = 17, 20, 9
    p = pc.problem(101, P, D, E, var)
    w = torch.tensor(p["w"].astype(np.float64), requires_grad=True)
    b = torch.tensor(p["b"].astype(np.float64), requires_grad=True)
    opt = (torch.optim.AdamW if var["decoupled"] else torch.optim.Adam)([w, b], lr=1e-3, weight_decay=var["weight_decay"], amsgrad=var["amsgrad"])
    idx = np.concatenate([p["left"], p["right"]])
    xb = torch.tensor(p["x"].astype(np.float64)[idx])
    if p["keep"] is not None:
        xb = xb * torch.tensor(p["keep"].astype(np.float64)) * pc.keep_scale(var)
    rw, rb, st = p["w"].astype(np.float64), p["b"].astype(np.float64), None
    for s in range(25):
        kw = pc.step_kw(var, s)
        for g in opt.param_groups:
            g["lr"] = kw["lr"]
        opt.zero_grad()
        per, _ = _torch_loss(F.linear(xb, w, b), p["differ"], P, pc.MARGIN, pc.W_SAME, pc.W_DIFF)
        loss = per.mean()
        loss.backward()
        opt.step()
        r = _rule_step(p, var, s, rw, rb, st, np.float64)
        rw, rb, st = r["w"], r["b"], r["state"]
        assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach()))), (s, r["loss"])
        assert np.abs(rw - w.detach().numpy()).max() <= 1e-12 and np.abs(rb - b.detach().numpy()).max() <= 1e-12, s
    assert st["t"] == 25 and st["rows"] == 25 * P


@pytest.mark.parametrize("E", (1, 2, 65, 256))
def test_closed_form_gradient_against_autograd(E):
    """Loss and ga of `pair_loss_rule` against autograd of the reference-shaped chain on `a`: normalise once and twice (the same
    gradient: the projection is idempotent), a pair of identical rows, and - under the single normalise - a zero row."""
    rng = np.random.default_rng(7 + E)
    P = 6
    al, ar = rng.standard_normal((P, E)), rng.standard_normal((P, E)) * 3
    ar[2] = al[2]
    differ = np.array([0, 1, 1, 0, 1, 0])
    for zero_row, twice in ((False, False), (False, True), (True, False)):
        if zero_row:
            al[4] = 0.0
        a = torch.tensor(np.concatenate([al, ar]), requires_grad=True)
        per, d = _torch_loss(a, differ, P, pc.MARGIN, pc.W_SAME, pc.W_DIFF, twice)
        per.mean().backward()
        loss, dist, gl, gr = hf.pair_loss_rule(al, ar, differ, P, pc.MARGIN, pc.W_SAME, pc.W_DIFF)
        want = a.grad.numpy()
        # (relative to the terms that cancel in it, q delta / s ~ 1 / (P s): with E = 1 the gradient itself is exactly zero)
        scale = max(np.abs(want).max(), 1.0 / (P * float(np.sqrt((np.concatenate([al, ar]) ** 2).sum(axis=1)).clip(1e-12).min())))
        assert np.abs(loss - per.detach().numpy()).max() <= 1e-12 and np.abs(dist - d.detach().numpy()).max() <= 1e-12
        assert np.abs(np.concatenate([gl, gr]) - want).max() <= 1e-12 * scale, (E, zero_row, twice)
        if zero_row:
            assert np.abs(gl[4]).max() > 1e6                                       # gd / 1e-12: the clamp of F.normalize passes it on


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the reference's own class
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rule_against_the_reference_contrastive_loss():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "contrastive_loss.json")))
    assert len(doc["cases"]) >= 8
    seen = set()
    for c in doc["cases"]:
        al, ar, label = np.array(c["a_l"]), np.array(c["a_r"]), np.array(c["label"])
        P = len(label)
        loss, dist, gl, gr = hf.pair_loss_rule(al, ar, label, P, c["margin"], c["neg_weight"], c["pos_weight"])   # (label 1: pushed apart)
        assert abs(loss.mean() - c["loss"]) <= 1e-12 * max(1.0, abs(c["loss"]))
        assert np.abs(np.maximum(dist, 1e-8) - np.maximum(np.array(c["dist"]), 1e-8)).max() <= 1e-12
        for got, want in ((gl, np.array(c["grad_l"])), (gr, np.array(c["grad_r"]))):
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        seen.add((al.shape[1], c["margin"]))
    assert {(1, 2.0), (65, 2.0), (5, 0.7)} <= seen


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the host twin against the float32 rule
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[pc.case_id(c) for c in CASES])
def test_twin_against_the_float32_rule(case):
    """a, row_src, w, b, the moments and the figures word for word (the rule takes the twin's own ga, pair_loss and dist for what lies
    downstream of them); ga, pair_loss and dist within one fp32 unit in the last place of the float64 evaluation."""
    (P, D, E), var = case
    p = pc.problem(pc.case_seed(case), P, D, E, var)
    if P >= 4:
        assert p["left"][0] == p["left"][1] and p["left"][2] == p["right"][2] and set(p["differ"].tolist()) == {0, 1}
    w, b = p["w"].copy(), p["b"].copy()
    st = np.zeros(hf.pair_state_bytes(D, E, var["amsgrad"]), np.uint8)
    rw, rb, rst = p["w"].copy(), p["b"].copy(), None
    worst = 0.0
    for s in range(pc.STEPS):
        what = "%s step %d" % (pc.case_id(case), s)
        ws = hf.pair_workspace_views(_host_step(p, var, s, w, b, st), P, E)
        own = _rule_step(p, var, s, rw, rb, rst, F32)
        pc.assert_no_knife_edge(hf.pair_loss_rule(own["a"][:P], own["a"][P:], p["differ"], max(own["n"], 1), *pc.LOSS_F32)[1], what)
        _same(ws["a"], own["a"], what + ": a")
        _same(ws["row_src"], own["row_src"], what + ": row_src")
        loss64, d64, gl, gr = hf.pair_loss_rule(ws["a"][:P], ws["a"][P:], p["differ"], own["n"], *pc.LOSS_F32)
        worst = max(worst, within_one_ulp(ws["ga"], np.concatenate([gl, gr]), what + ": ga"),
                    within_one_ulp(ws["pair_loss"], loss64, what + ": pair_loss"), within_one_ulp(ws["dist"], d64, what + ": dist"))
        r = _rule_step(p, var, s, rw, rb, rst, F32, given={k: ws[k] for k in ("a", "ga", "pair_loss", "dist")})
        rw, rb, rst = r["w"], r["b"], r["state"]
        _same(w, rw, what + ": w")
        _same(b, rb, what + ": b")
        v = hf.state_views(st, D, E, var["amsgrad"])
        for k in hf.HEADER:
            assert int(v[k]) == rst[k], (what, k, int(v[k]), rst[k])
        for k in ("m_w", "v_w", "m_b", "v_b") + (("vmax_w", "vmax_b") if var["amsgrad"] else ()):
            _same(v[k], rst[k], what + ": " + k)
    assert rst["t"] == pc.STEPS and rst["n"] == P and rst["rows"] == pc.STEPS * P and not np.array_equal(w, p["w"])
    print("%s: worst ga / pair_loss / dist %.3f ulp" % (pc.case_id(case), worst))


def test_no_gpu_only_case_has_a_knife_edge():
    """The cases only the GPU file runs, walked here with the twin: no pair within 1e-4 of accept or margin at any of the three steps,
    and every one holds what a case must hold."""
    for case in [c for c in pc.cases(pc.GPU_SHAPES) if c not in CASES]:
        (P, D, E), var = case
        p = pc.problem(pc.case_seed(case), P, D, E, var)
        assert p["left"][0] == p["left"][1] and p["left"][2] == p["right"][2] and set(p["differ"].tolist()) == {0, 1}
        w, b, st = p["w"].copy(), p["b"].copy(), np.zeros(hf.pair_state_bytes(D, E, var["amsgrad"]), np.uint8)
        for s in range(pc.STEPS):
            a = hf.pair_workspace_views(_host_step(p, var, s, w, b, st), P, E)["a"]
            pc.assert_no_knife_edge(hf.pair_loss_rule(a[:P], a[P:], p["differ"], P, *pc.LOSS_F32)[1], "%s step %d" % (pc.case_id(case), s))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. bad pairs, the all-declined batch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.BAD_KINDS)
def test_a_bad_pair_counts_for_nothing(kind):
    """The batch with the bad pair inserted against the batch without it: the twin's w, b and state hold the same bytes (2P <= 128:
    one chain, and a +0 row is a no-op in it), the float64 rule agrees to 1e-12, and the pair's workspace rows are empty."""
    P, D, E = 17, 65, 33
    for var in pc.VARIATIONS:
        p = pc.problem(1200, P, D, E, var)
        q = pc.with_bad_pair(p, kind, 5)
        out = []
        for prob in (p, q):
            w, b, st = prob["w"].copy(), prob["b"].copy(), np.zeros(hf.pair_state_bytes(D, E, var["amsgrad"]), np.uint8)
            for s in range(2):
                ws = _host_step(prob, var, s, w, b, st)
            out.append((w, b, st, hf.pair_workspace_views(ws, prob["P"], E)))
        for k, name in enumerate(("w", "b", "state")):
            _same(out[0][k], out[1][k], "%s, %s: %s" % (kind, var["name"], name))
        v = out[1][3]
        assert v["row_src"][5] == -1 and v["row_src"][P + 1 + 5] == -1 and (v["row_src"][[4, 6]] >= 0).all()
        assert not v["ga"][5].any() and not v["ga"][P + 1 + 5].any() and np.isnan(v["pair_loss"][5]) and np.isnan(v["dist"][5])
        assert int(st[8:16].view(np.uint64)[0]) == P
        good = np.delete(np.arange(P + 1), 5)
        _same(v["ga"][good], out[0][3]["ga"][:P], "%s: ga of the left rows of the other pairs" % kind)
        a, c = (_rule_step(prob, var, 0, prob["w"], prob["b"], None, np.float64) for prob in (p, q))
        assert c["n"] == P and np.abs(a["w"] - c["w"]).max() <= 1e-12 and np.abs(a["b"] - c["b"]).max() <= 1e-12
        assert abs(a["loss"] - c["loss"]) <= 1e-12 and a["state"]["correct"] == c["state"]["correct"]
        # the half of the pair that is fine keeps its projection
        fine = P + 1 + 5 if kind in ("left -1", "nan feature") else 5
        if not kind.startswith("differ") and kind != "inf feature" and kind != "right N":
            assert v["a"][fine].any() and not v["a"][5].any()


def test_an_all_declined_batch_changes_nothing_but_the_workspace():
    P, D, E = 9, 12, 7
    var = pc.VARIATIONS[1]
    p = pc.problem(1300, P, D, E, var)
    w, b, st = p["w"].copy(), p["b"].copy(), np.zeros(hf.pair_state_bytes(D, E, True), np.uint8)
    _host_step(p, var, 0, w, b, st)
    before = (w.copy(), b.copy(), st.copy())
    dead = dict(p, differ=np.full(P, 2, np.int32))
    dead["left"] = p["left"].copy()
    dead["left"][::2] = -1
    ws = np.full(hf.pair_workspace_bytes(P, D, E), 0x5A, np.uint8)
    _host_step(dead, var, 1, w, b, st, ws, clear=False)
    _same(w, before[0], "w")
    _same(b, before[1], "b")
    changed = np.flatnonzero(st != before[2])
    assert set(changed.tolist()) <= set(range(8, 16)) and int(st[8:16].view(np.uint64)[0]) == 0 and int(st[:8].view(np.uint64)[0]) == 1
    v = hf.pair_workspace_views(ws, P, E)
    assert (v["row_src"] == -1).all() and not v["ga"].any() and np.isnan(v["pair_loss"]).all() and np.isnan(v["dist"]).all()
    assert v["a"][1].any() and not v["a"][0].any()                               # a counted ROW of an uncounted pair keeps its projection
    r = _rule_step(dead, var, 1, before[0], before[1], None, F32, clear=False)
    assert r["n"] == 0 and np.array_equal(r["w"], before[0]) and r["state"]["t"] == 0 and math.isnan(r["loss"])
    _same(v["a"], r["a"], "a of the all-declined batch")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pair_entry_points_are_declared_bound_and_element_aligned():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_head_fit_pair_state_bytes", 3), ("frmap_head_fit_pair_workspace_bytes", 3),
                       ("frmap_head_fit_pair_step", 25), ("frmap_head_fit_pair_step_host", 25)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10          # only symbols are added
    rows = _lib.ALIGNMENT["frmap_head_fit_pair_step"]
    assert list(rows) == ["x", "left", "right", "differ", "keep", "w", "b", "state", "workspace"]
    assert all(cls == "element" for cls, _ in rows.values())
    assert [n for _, n in rows.values()] == [4, 4, 4, 4, 1, 4, 4, 8, 4]
    assert "frmap_head_fit_pair_step_host" not in _lib.ALIGNMENT
    assert {"frmap_head_fit_pair_state_bytes", "frmap_head_fit_pair_workspace_bytes"} <= set(oc.pointer_free())
    for name in ("pair_state_bytes", "pair_workspace_bytes", "pair_step", "pair_step_host", "pair_step_rule", "PairHead", "draw_pairs",
                 "cache_embeddings", "fit_pair_head"):
        assert callable(getattr(hf, name)), name


def test_pair_sizes():
    lib = _lib.load()
    for D, E in ((1, 1), (3, 2), (512, 256), (65, 33)):
        for ams in (0, 1):
            assert lib.frmap_head_fit_pair_state_bytes(D, E, ams) == lib.frmap_head_fit_state_bytes(D, E, ams) == hf.pair_state_bytes(D, E, bool(ams))
        for P in (1, 16, 33):
            assert lib.frmap_head_fit_pair_workspace_bytes(P, D, E) == 4 * (4 * P * E + 4 * P) == hf.pair_workspace_bytes(P, D, E)
            v = hf.pair_workspace_views(np.zeros(hf.pair_workspace_bytes(P, D, E), np.uint8), P, E)
            assert v["a"].shape == v["ga"].shape == (2 * P, E) and v["pair_loss"].shape == v["dist"].shape == (P,) and v["row_src"].shape == (2 * P,)
    for bad in ((0, 1), (1, 0), (65537, 1), (1, 65537)):
        assert lib.frmap_head_fit_pair_state_bytes(*bad, 0) == 0 and lib.frmap_head_fit_pair_workspace_bytes(4, *bad) == 0, bad
    assert lib.frmap_head_fit_pair_workspace_bytes(0, 2, 2) == 0 and lib.frmap_head_fit_pair_workspace_bytes(2 ** 19 + 1, 2, 2) == 0
    assert lib.frmap_head_fit_pair_workspace_bytes(2 ** 19, 2, 65536) == 4 * (4 * 2 ** 35 + 4 * 2 ** 19)
    with pytest.raises(ValueError, match="E = 0"):
        hf.pair_state_bytes(2, 0)
    with pytest.raises(ValueError, match="P = 0"):
        hf.pair_workspace_bytes(0, 2, 2)


def test_twin_and_launcher_refusals_name_the_argument():
    """Both come before anything is read, written or launched: host dummy pointers serve."""
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.uint8)
    p = (buf.ctypes.data + 255) // 256 * 256
    ok = dict(x=p, left=p, right=p, differ=p, keep=0, ks=1.0, w=p, b=p, state=p, workspace=p, N=1, P=1, D=1, E=1, flags=0)
    floats = (2.0, 0.8, 1.2, 0.5, 1e-3, 0.9, 0.999, 1e-8, 0.0)

    def args(**kw):
        a = dict(ok, **kw)
        return [a[k] for k in ("x", "left", "right", "differ", "keep", "ks", "w", "b", "state", "workspace", "N", "P", "D", "E")] + list(floats) + [a["flags"]]
    refused = [(dict(flags=8), "flags"), (dict(N=0), "N"), (dict(P=0), "P"), (dict(P=2 ** 19 + 1), "P"), (dict(D=0), "D"), (dict(D=65537), "D"),
               (dict(E=0), "E"), (dict(E=65537), "E"), (dict(N=0, P=0), "N"), (dict(P=0, D=0), "P"), (dict(D=0, E=0), "D"),
               (dict(E=0, flags=8), "E"), (dict(flags=8, w=0), "flags"), (dict(x=0), "null pointer"), (dict(left=0), "null pointer"),
               (dict(right=0), "null pointer"), (dict(differ=0), "null pointer"), (dict(w=0), "null pointer"), (dict(b=0), "null pointer"),
               (dict(state=0), "null pointer"), (dict(workspace=0), "null pointer")]
    for kw, word in refused:
        for name, fn, last in (("head_fit_pair_step_host", lib.frmap_head_fit_pair_step_host, 0), ("head_fit_pair_step", lib.frmap_head_fit_pair_step, None)):
            assert fn(*args(**kw), last) == -1, (name, kw)
            msg = lib.frmap_last_error().decode()
            assert msg.startswith(name + ": ") and oc.names_operand(msg, word.split()[0]), (name, kw, msg)
            assert msg[len(name) + 2:].startswith(word), (name, kw, msg)            # the FIRST failing check of the shared order
    for arg, need in (("x", 4), ("left", 4), ("right", 4), ("differ", 4), ("w", 4), ("b", 4), ("state", 8), ("workspace", 4)):
        assert lib.frmap_head_fit_pair_step(*args(**{arg: p + need // 2}), None) == -1, arg
        msg = lib.frmap_last_error().decode()
        assert msg.startswith("head_fit_pair_step: ") and "%s must be %d-byte aligned" % (arg, need) in msg, (arg, msg)
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
    N, P, D, E = 9, 4, 8, 6
    g = torch.Generator().manual_seed(1)
    return dict(x=torch.randn((N, D), generator=g), left=torch.tensor([0, 3, 8, -1], dtype=torch.int32),
                right=torch.tensor([1, 3, 2, 5], dtype=torch.int32), differ=torch.tensor([0, 1, 1, 0], dtype=torch.int32),
                w=torch.randn((E, D), generator=g), b=torch.zeros((E,)),
                state=torch.zeros((hf.pair_state_bytes(D, E, amsgrad),), dtype=torch.uint8),
                workspace=torch.zeros((hf.pair_workspace_bytes(P, D, E),), dtype=torch.uint8), keep=torch.ones((2 * P, D), dtype=torch.uint8))


ORDER = ("x", "left", "right", "differ", "w", "b", "state", "workspace", "keep")
# the axes along which an operand's extent is another operand's (w's first axis GIVES E, left's P)
DEPENDENT = {"right": (0,), "differ": (0,), "w": (1,), "b": (0,), "state": (0,), "workspace": (0,), "keep": (0, 1)}


def _call(values, **kw):
    return hf.pair_step(*[_gpu(values[k]) for k in ORDER], 1.0, **kw)


def test_the_valid_pair_call_reaches_the_library(stub):
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(_valid())
    assert e.value.entry == "frmap_head_fit_pair_step" and e.value.args_[10:14] == (9, 4, 8, 6) and e.value.args_[23] == 0
    assert e.value.args_[14:18] == (2.0, 0.8, 1.2, 0.5) and len(stub.calls) == 1
    v = _valid(True)
    v["keep"] = None
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(v, amsgrad=True, clear=True, decoupled=True, margin=1.5)
    assert e.value.args_[4] == 0 and e.value.args_[23] == 7 and e.value.args_[14] == 1.5


@pytest.mark.parametrize("operand", sorted(DEPENDENT))
def test_a_dependent_pair_operand_is_refused_before_the_library(operand, stub):
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
    with pytest.raises(RuntimeError) as e:                                       # this one stays a CPU tensor
        hf.pair_step(*[values[k] if k == operand else _gpu(values[k]) for k in ORDER], 1.0)
    assert oc.names_operand(str(e.value), operand)
    assert stub.calls == []


def test_free_pair_operands_are_refused(stub):
    for operand, bad, exc in (("x", torch.zeros((9,)), ValueError), ("x", torch.zeros((9, 8), dtype=torch.float64), TypeError),
                              ("left", torch.zeros((2, 2), dtype=torch.int32), ValueError), ("left", None, ValueError),
                              ("left", torch.zeros((4,), dtype=torch.int64), TypeError), ("w", None, TypeError)):
        values = _valid()
        values[operand] = bad
        with pytest.raises(exc):
            _call(values)
    with pytest.raises(ValueError, match="state"):                    # the AMSGrad state is larger
        _call(_valid(), amsgrad=True)
    with pytest.raises(ValueError):
        hf.PairHead(8, 0, "cpu")
    with pytest.raises(ValueError):
        hf.PairHead(hf.MAX_D + 1, 4, "cpu")
    assert stub.calls == []


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. PairHead, draw_pairs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pair_head_initialises_as_a_linear_head():
    D, E = 16, 12
    head = hf.PairHead(D, E, "cpu", amsgrad=True, generator=torch.Generator().manual_seed(7))
    lin = hf.LinearHead(D, E, "cpu", amsgrad=True, generator=torch.Generator().manual_seed(7))
    torch.manual_seed(7)
    ref = torch.nn.Linear(D, E)
    assert torch.equal(head.weight, lin.weight) and torch.equal(head.bias, lin.bias) and torch.equal(head.weight, ref.weight.detach())
    assert head.state.numel() == hf.pair_state_bytes(D, E, True) == lin.state.numel() and not head.state.any()
    fig = head.epoch_figures()
    assert fig["rows"] == 0 and fig["t"] == 0 and np.isnan(fig["accuracy"]) and np.isnan(fig["loss"])
    assert sorted(head.state_dict()) == ["bias", "weight"]
    import frmap_amd
    model = frmap_amd.get_model("siamese", 4)
    with pytest.raises(ValueError, match="fc.8"):
        head.load_into(model)                                         # fc.8 is [256, 512]
    with pytest.raises(ValueError, match="BaselineNet"):
        head.load_into(frmap_amd.get_model("baseline", 4))
    own = hf.PairHead(512, 256, "cpu", generator=torch.Generator().manual_seed(3))
    own.load_into(model)
    assert torch.equal(model.fc[8].weight.detach(), own.weight) and torch.equal(model.fc[8].bias.detach(), own.bias)
    with pytest.raises(ValueError, match="fc_hidden"):
        hf.cache_embeddings(frmap_amd.get_model("baseline", 4), [], layer="fc_hidden")
    with pytest.raises(ValueError, match="layer"):
        hf.cache_embeddings(model, [], layer="pooled")
    # the classifier entries keep their refusal of a siamese model word for word
    for fn in (lambda: hf.cache_features(model, "siamese", []), lambda: hf.fit_head(model, "siamese", [])):
        with pytest.raises(ValueError, match=re.escape("head_fit: a siamese model has no classifier head to fit (pairs are verification_metrics' business)")):
            fn()


def test_draw_pairs():
    g = torch.Generator().manual_seed(11)
    labels = torch.tensor([5] * 40 + [2] * 30 + [9] + [7] * 29, dtype=torch.int32)[torch.randperm(100, generator=g)]
    P = 20000
    left, right, differ = hf.draw_pairs(labels, P, g)
    assert left.dtype == right.dtype == differ.dtype == torch.int32 and left.shape == right.shape == differ.shape == (P,)
    assert int(left.min()) >= 0 and int(left.max()) < 100 and int(right.min()) >= 0 and int(right.max()) < 100
    ll, lr = labels[left.long()], labels[right.long()]
    assert torch.equal(differ, (ll != lr).to(torch.int32)) and not bool((left == right).any())
    lone = int((labels == 9).nonzero()[0])
    assert bool(differ[left == lone].all()) and bool(differ[right == lone].all()) and int((left == lone).sum()) > 0
    # anchors uniform over 100 rows: each row 200 +- 5 sigma (sigma = sqrt(P * .01 * .99) = 14.1)
    counts = torch.bincount(left.long(), minlength=100)
    assert int(counts.min()) >= 200 - 71 and int(counts.max()) <= 200 + 71
    # the same-pair share: 99% of the anchors have a classmate, half of those draw it: 0.495 P, sigma = sqrt(P / 4) = 70.7
    same = int((differ == 0).sum())
    assert abs(same - 0.495 * P) <= 5 * 70.7, same
    # partners of a same pair are uniform over the OTHER rows of the class, of a different pair over the rows of other classes
    a = int((labels == 2).nonzero()[0])
    mates = right[(left == a) & (differ == 0)].long()
    others = right[(left == a) & (differ == 1)].long()
    assert set(mates.tolist()) <= set((labels == 2).nonzero().flatten().tolist()) - {a} and len(set(mates.tolist())) >= 20
    assert len(set(others.tolist())) >= 40 and not bool((labels[others] == 2).any())
    # the same seed, the same pairs; a single class: same pairs only; refusals
    again = hf.draw_pairs(labels, P, torch.Generator().manual_seed(11))
    g2 = torch.Generator().manual_seed(11)
    torch.randperm(100, generator=g2)
    for u, v in zip(hf.draw_pairs(labels, P, g2), (left, right, differ)):
        assert torch.equal(u, v)
    assert again[0].shape == (P,)
    l1, r1, d1 = hf.draw_pairs(torch.zeros(5, dtype=torch.int64), 50, g)
    assert not bool(d1.any()) and not bool((l1 == r1).any())
    l2, r2, d2 = hf.draw_pairs(torch.arange(6), 50, g)
    assert bool(d2.all()) and not bool((l2 == r2).any())
    for bad in (lambda: hf.draw_pairs(torch.zeros(1, dtype=torch.int32), 4), lambda: hf.draw_pairs(labels, 0),
                lambda: hf.draw_pairs(labels.float(), 4), lambda: hf.draw_pairs(labels[None], 4)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the synthetic fit with the float32 rule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_float32_rule_learns_the_synthetic_embedding():
    """`fit_pair_cases.FIT` at its pinned seed: the validation EER of normalize(x w^T + b) after 300 steps of the float32 rule is at most
    one third of the raw features' EER.  Measured at seed 3: raw 0.4745, fitted 0.0935 (0.197 of raw)."""
    f = pc.FIT
    xt, yt, xv, yv, steps = pc.fit_data()
    w, b = (t.numpy() for t in hf._linear_init(f["E"], f["D"], torch.Generator().manual_seed(f["seed"])))
    raw = pc.eer(xv, yv)
    st = None
    for left, right, differ in steps:
        r = hf.pair_step_rule(xt, left, right, differ, w, b, st, lr=f["lr"], dtype=F32)
        w, b, st = r["w"], r["b"], r["state"]
    fitted = pc.eer(pc.unit(xv.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)), yv)
    print("synthetic fit, float32 rule: raw EER %.4f, fitted EER %.4f, train accuracy %.3f" % (raw, fitted, st["correct"] / st["rows"]))
    assert st["t"] == f["steps"] and st["rows"] == f["steps"] * f["pairs"]
    assert fitted <= raw / 3, (raw, fitted)


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the check program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_pair_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/head_fit_pair_check.cpp (its own `main`, head_fit_twin.h, the two rule headers and tools/head_fit_check_common.h, nothing
    else) built with -fsanitize=address,undefined (runtimes linked statically) and run directly as a child process: it sweeps the CPU
    table of `fit_pair_cases` with every buffer a heap block of exactly its size, and exits 0."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "head_fit_pair_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    src_path = os.path.join(ROOT, "tools", "head_fit_pair_check.cpp")
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc, src_path, "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.stdout.splitlines()[-2:] == ["%d cases" % len(CASES), "self check passed"], run.stdout[-500:]
    src = open(src_path).read()                                                  # the program's table is this module's
    assert "shapes[][3] = {%s}" % ", ".join("{%d, %d, %d}" % s for s in pc.CPU_SHAPES) in src
