"""CPU: the margin head-fitting step - a first step worked by hand, the float64 rule (`head_fit.margin_step_rule`) against torch autograd
through the reference's call sequence over 25 steps, against the reference's own ArcMarginProduct (tests/golden/arc_margin.json) with
`head_fit.margin_schedule` against its recorded factors, the host twin (`head_fit.margin_step_host`) against the float32 rule over
the 125 shapes of `fit_margin_cases` (where the knife-edge conditions of every table are asserted too), the hand-built branch rows,
declined rows, the all-declined batch, the C ABI of the four entry points, the refusals of `head_fit.margin_step` under
`operand_cases`' stub (nothing launches), `MarginHead`'s initialisation and `load_into`, the synthetic fit with the float32 rule, and
tools/head_fit_margin_check.cpp under the address and undefined-behaviour sanitizers."""
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

import fit_margin_cases as mc
import operand_cases as oc
from frmap_amd import _lib, head_fit as hf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GIVEN = ("z", "rx", "rw", "cosv", "g", "h", "row_loss")
ROUNDED = ("rx", "rw", "cosv", "g", "h", "row_loss")


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


def exact_halves(x, labels, w, v, rows, keep, keep_scale, kw):
    """The float64 value of every rounded quantity of a step FROM THE INPUTS IT IS ROUNDED FROM: rx and rw from x' and w, and cosv, g, h
    and the row loss from the fp32 ``z``, ``rx`` and ``rw`` of the workspace views ``v``."""
    x32, lab = np.asarray(x, F32), np.asarray(labels).astype(np.int64)
    B = len(rows) if rows is not None else (len(keep) if keep is not None else kw.get("batch") or len(x32))
    row_src, ok, xp = hf._rule_batch(x32, lab, w.shape[0], rows, B, keep, keep_scale, True)
    r = {"y": np.where(ok, lab[np.clip(row_src, 0, len(x32) - 1)], 0), "n": int(ok.sum())}
    rx = np.where(ok, 1.0 / np.maximum(np.sqrt((xp.astype(np.float64) ** 2).sum(axis=1)), 1e-12), 0.0)
    rw = 1.0 / np.maximum(np.sqrt((np.asarray(w, np.float64) ** 2).sum(axis=1)), 1e-12)
    det = hf.margin_logits_rule(v["z"], v["rx"], v["rw"], r["y"], float(F32(kw["s"])), float(F32(kw["m"])), kw["easy_margin"], True)
    l = det["l"]
    B, C = l.shape
    ls = float(F32(kw["label_smoothing"]))
    with np.errstate(all="ignore"):
        mx = l.max(axis=1, keepdims=True)
        e = np.exp(l - mx)
        sm = e.sum(axis=1, keepdims=True)
        nl = np.log(sm) - (l - mx)
        off = ls / C if ls > 0 else 0.0
        loss = (1.0 - ls) * nl[np.arange(B), r["y"]] + off * nl.sum(axis=1) if ls > 0 else nl[np.arange(B), r["y"]]
        loss = np.where(ok, np.maximum(loss, 0.0), np.nan)
        t = np.full((B, C), off)
        t[np.arange(B), r["y"]] = (1.0 - ls) + off
        gcos = ((float(F32(kw["s"])) * (e / sm - t)) / max(r["n"], 1)) * det["dfac"]
        g = np.where(ok[:, None], gcos * v["rx"].astype(np.float64)[:, None], 0.0)
        h = np.where(ok[:, None], gcos * det["cos"], 0.0)
        cosv = np.where(ok[:, None], det["cs"], 0.0)
    return {"rx": rx, "rw": rw, "cosv": cosv, "g": g, "h": h, "row_loss": loss}


def _host_step(p, var, k, w, st, ws=None, given_g=False, clear=None, **over):
    return hf.margin_step_host(p["x"], p["labels"], w, st, ws, p["rows"], p["keep"], mc.keep_scale(var), given_g=given_g,
                               **dict(mc.step_kw(var, k, clear), **over))


def _rule_step(p, var, k, w, state, dtype, clear=None, given=None, **over):
    return hf.margin_step_rule(p["x"], p["labels"], w, state, p["rows"], p["keep"], mc.keep_scale(var), dtype=dtype, given=given,
                               **dict(mc.step_kw(var, k, clear), **over))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. a first step by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_first_step_by_hand():
    """One row x = (3, 4), label 0, the centres w_0 = (4, 3) and w_1 = (0, 5): every norm is 5, so rx = rw = 0.2, z = (24, 20) and
    cos = (0.96, 0.8), sin theta_0 = 0.28.  The margin m = atan2(0.6, 0.8) has cos m = 0.8, sin m = 0.6, so cos(theta_0 + m) =
    0.96 x 0.8 - 0.28 x 0.6 = 0.6, sin(theta_0 + m) = 0.28 x 0.8 + 0.96 x 0.6 = 0.8 and dfac_0 = 0.8 / 0.28.  With s = 5 the logits are
    (3, 4): p = (1 / (1 + e), e / (1 + e)), the loss is log(1 + e) = 1.3132616875..., q = 5 (p - y) = (-3.6552928931, 3.6552928931),
    gcos = (q_0 / 0.35, q_1), g = 0.2 gcos, h = (0.96 gcos_0, 0.8 gcos_1), and
    dw_0 = 0.2 g_0 (3, 4) - 0.04 h_0 (4, 3) = (0.3509081170, -0.4678774894), orthogonal to w_0;
    dw_1 = 0.2 g_1 (3, 4) - 0.04 h_1 (0, 5) = (0.4386351472, 0), orthogonal to w_1.
    Adam's first step moves a weight by lr against the sign of its gradient (where that is not a rounding residue)."""
    x, labels, w = np.array([[3.0, 4.0]]), np.array([0]), np.array([[4.0, 3.0], [0.0, 5.0]])
    m = math.atan2(0.6, 0.8)
    r = hf.margin_step_rule(x, labels, w, s=5.0, m=m, lr=0.1)
    e = math.e
    q1 = 5.0 * e / (1.0 + e)
    np.testing.assert_allclose(r["z"], [[24.0, 20.0]], rtol=0, atol=0)
    np.testing.assert_allclose(r["rx"], [0.2], rtol=1e-15)
    np.testing.assert_allclose(r["rw"], [0.2, 0.2], rtol=1e-15)
    np.testing.assert_allclose(r["detail"]["out"], [[0.6, 0.8]], rtol=1e-14)
    np.testing.assert_allclose(r["detail"]["dfac"], [[0.8 / 0.28, 1.0]], rtol=1e-13)
    np.testing.assert_allclose(r["row_loss"], [1.3132616875182228], rtol=1e-14)
    np.testing.assert_allclose(q1, 3.6552928931500244, rtol=1e-14)
    np.testing.assert_allclose(r["g"], [[-0.2 * q1 / 0.35, 0.2 * q1]], rtol=1e-13)
    np.testing.assert_allclose(r["g"], [[-2.0887387960857283, 0.7310585786300049]], rtol=1e-13)
    np.testing.assert_allclose(r["h"], [[-0.96 * q1 / 0.35, 0.8 * q1]], rtol=1e-13)
    np.testing.assert_allclose(r["dw"], [[0.35090811774240236, -0.46787749032320315], [0.43863514717800293, 0.0]], rtol=1e-12, atol=1e-14)
    assert abs(float(r["dw"][0] @ w[0])) < 1e-14 and abs(float(r["dw"][1] @ w[1])) < 1e-14
    np.testing.assert_allclose(r["w"][0], [3.9, 3.1], rtol=1e-7)
    np.testing.assert_allclose(r["w"][1, 0], -0.1, rtol=1e-7)
    assert r["n"] == 1 and r["state"]["t"] == 1 and r["state"]["correct"] == 0 and int(r["pred"][0]) == 1
    # the float32 rule and the twin on the same numbers (m is taken as fp32: parts in 1e-8)
    r32 = hf.margin_step_rule(x, labels, w, s=5.0, m=m, lr=0.1, dtype=F32)
    w32, st = w.astype(F32), np.zeros(hf.margin_state_bytes(2, 2), np.uint8)
    v = hf.margin_workspace_views(hf.margin_step_host(x, labels, w32, st, s=5.0, m=m, lr=0.1), 1, 2)
    for k in ("g", "h", "row_loss", "cosv"):
        np.testing.assert_allclose(v[k], r32[k], rtol=2e-7)
        np.testing.assert_allclose(r32[k], r[k] if k != "cosv" else [[0.96, 0.8]], rtol=1e-6)
    np.testing.assert_allclose(w32[0], [3.9, 3.1], rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the float64 rule against torch
# ---------------------------------------------------------------------------------------------------------------------------------
def _torch_logits(xt, wt, lab, s, m, easy):
    """The reference's sequence of calls (`src/face_models.py:351-412`) on float64 tensors."""
    xn, wn = F.normalize(xt, p=2, dim=1, eps=1e-12), F.normalize(wt, p=2, dim=1, eps=1e-12)
    cs = torch.clamp(F.linear(xn, wn), min=-1.0 + 1e-7, max=1.0 - 1e-7)
    theta = torch.acos(cs)
    if easy:
        phi = torch.where(cs > 0, torch.cos(theta + m), cs)
    else:
        phi = torch.cos(torch.minimum(torch.tensor(math.pi - 1e-4), theta + m))
    one_hot = torch.zeros_like(cs)
    one_hot.scatter_(1, lab.view(-1, 1), 1)
    return torch.where(one_hot.bool(), phi, cs) * s


TORCH_CASES = (
    dict(shape=(6, 8, 5), decoupled=False, amsgrad=False, ls=0.0, keep=False, easy=False),
    dict(shape=(33, 65, 18), decoupled=True, amsgrad=True, ls=0.05, keep=True, easy=False),
    dict(shape=(16, 3, 2), decoupled=True, amsgrad=False, ls=0.05, keep=False, easy=True),
    dict(shape=(9, 130, 33), decoupled=False, amsgrad=True, ls=0.0, keep=True, easy=True),
)


@pytest.mark.parametrize("case", TORCH_CASES, ids=["-".join(map(str, c["shape"])) + ("-easy" if c["easy"] else "") for c in TORCH_CASES])
def test_float64_rule_against_torch_over_25_steps(case):
    """F.normalize -> F.linear -> clamp -> acos -> minimum / where -> cross_entropy(label_smoothing=) -> Adam / AdamW, in float64, with
    the schedule's scale and margin changing every step, a fresh batch and (where the case has one) a fresh dropout mask per step, a
    capped target (row 0 is -1.5 w_y at the start), a clamped element (row 1 is 2 w_y) and a zero class centre.  Loss and weights
    agree to 1e-12."""
    B, D, C = case["shape"]
    rng = np.random.default_rng(77 + B)
    N = B + 4
    x = rng.standard_normal((N, D))
    labels = rng.integers(0, C, N)
    w = rng.standard_normal((C, D)) * math.sqrt(4.0 / (C + D))
    w[C - 1] = 0.0
    x[0], x[1] = -1.5 * w[labels[0]], 2.0 * w[labels[1]]
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    opt = (torch.optim.AdamW if case["decoupled"] else torch.optim.Adam)([wt], lr=1e-2, weight_decay=1e-2, amsgrad=case["amsgrad"])
    st, worst = None, 0.0
    for k in range(25):
        m_eff, s_eff = hf.margin_schedule(k // 2, 32.0, 0.5)
        rows = np.concatenate([[0, 1], 2 + rng.permutation(N - 2)[:B - 2]]) if k < 2 else rng.permutation(N)[:B]
        keep = (rng.random((B, D)) >= 0.25).astype(np.uint8) if case["keep"] else None
        scale = 1.0 / 0.75 if case["keep"] else 1.0
        for g in opt.param_groups:
            g["lr"] = mc.LRS[k % 3]
        xb = torch.tensor(x[rows] * (keep * scale if keep is not None else 1.0), dtype=torch.float64)
        loss = F.cross_entropy(_torch_logits(xb, wt, torch.tensor(labels[rows]), s_eff, m_eff, case["easy"]), torch.tensor(labels[rows]),
                               label_smoothing=case["ls"])
        opt.zero_grad()
        loss.backward()
        r = hf.margin_step_rule(x, labels, w, st, rows=rows, keep=keep, keep_scale=scale, s=s_eff, m=m_eff, easy_margin=case["easy"],
                                lr=mc.LRS[k % 3], weight_decay=1e-2, label_smoothing=case["ls"], decoupled=case["decoupled"],
                                amsgrad=case["amsgrad"])
        gt = wt.grad.numpy()
        worst = max(worst, float(np.abs(r["dw"] - gt).max() / max(np.abs(gt).max(), 1e-300)))
        assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach()))), (k, r["loss"], float(loss.detach()))
        opt.step()
        w, st = r["w"], r["state"]
        np.testing.assert_allclose(w, wt.detach().numpy(), rtol=1e-12, atol=1e-12, err_msg="step %d" % k)
    print("float64 rule against torch, %s: worst relative gradient difference %.3g" % (case["shape"], worst))
    assert worst <= 1e-12 and st["t"] == 25


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the reference's own module
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rule_and_schedule_against_the_reference_module():
    with open(os.path.join(ROOT, "tests", "golden", "arc_margin.json")) as f:
        cases = json.load(f)["cases"]
    assert {c["epoch"] for c in cases} == {0, 3, 9, 10, 25} and {c["m"] for c in cases} == {0.3, 0.5} and {c["easy_margin"] for c in cases} == {False, True}
    capped = clamped = 0
    for c in cases:
        m_eff, s_eff = hf.margin_schedule(c["epoch"], c["s"], c["m"])
        progress = c["epoch"] / 10
        mf = min(0.9, progress * progress) if c["epoch"] < 10 else 0.9
        sf = min(0.8, 0.3 + 0.5 * progress) if c["epoch"] < 10 else 0.8
        assert mf == c["margin_factor"] and sf == c["scale_factor"], c["epoch"]              # exactly: the same arithmetic
        assert m_eff == c["m"] * c["margin_factor"]
        assert s_eff == min(c["s"], 24.0) * min(0.8, c["scale_factor"]) * ((0.8 - 0.5 * c["margin_factor"]) if c["m"] > 0.4 else 1.0)
        r = hf.margin_step_rule(np.array(c["input"]), np.array(c["label"]), np.array(c["weight"]), s=s_eff, m=m_eff, easy_margin=c["easy_margin"])
        out = np.array(c["output"])
        np.testing.assert_allclose(r["detail"]["l"], out, rtol=1e-12, atol=1e-12)
        mc.assert_no_knife_edge(r, c["easy_margin"], "golden epoch %d" % c["epoch"])
        capped += int((~np.array(c["easy_margin"]) & (r["detail"]["theta_m"] >= hf.MARGIN_CAP)).sum())
        clamped += int((~r["detail"]["inside"]).sum())
    assert capped >= 1 and clamped >= 1
    assert hf.margin_schedule(4, warm_up=False) == (0.0, 24.0 * 0.3 * 0.8)                      # the module's initial factors
    assert max(hf.margin_schedule(e, s, 0.3)[1] for e in range(40) for s in (8.0, 32.0, 64.0)) == 24.0 * 0.8 < 20.0   # the "hard cap" cannot fire


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the twin against the float32 rule; the knife-edge conditions of every table
# ---------------------------------------------------------------------------------------------------------------------------------
def run_twin_case(shape, steps=mc.STEPS):
    """`steps` steps of a shape through the twin, the float32 rule on the twin's own rounded values, and the float64 rule beside them
    (its own weights; the conditions and `correct` are checked on it).  Returns the worst deviations in fp32 units."""
    var = mc.variation(shape)
    p = mc.problem(mc.case_seed(shape), *shape, var)
    B, D, C = shape
    w = p["w"].copy()
    st = np.zeros(hf.margin_state_bytes(D, C, var["amsgrad"]), np.uint8)
    w_rule, st_rule, worst = p["w"].copy(), None, dict.fromkeys(ROUNDED, 0.0)
    for k in range(steps):
        kw = mc.step_kw(var, k)
        what = "%s step %d" % (mc.case_id(shape), k)
        r64 = _rule_step(p, var, k, w.astype(np.float64), None, np.float64, clear=False)
        mc.assert_no_knife_edge(r64, kw["easy_margin"], what)
        w_before = w.copy()
        v = hf.margin_workspace_views(_host_step(p, var, k, w, st), B, C)
        r = _rule_step(p, var, k, w_rule, st_rule, F32, given={g: v[g].copy() for g in GIVEN})
        own = _rule_step(p, var, k, w_rule, st_rule, F32)
        _same(v["z"], own["z"], what + ": z")
        _same(v["row_src"], r["row_src"], what + ": row_src")
        exact = exact_halves(p["x"], p["labels"], w_before, v, p["rows"], p["keep"], mc.keep_scale(var), kw)
        for g in ROUNDED:
            worst[g] = max(worst[g], within_one_ulp(v[g], exact[g], what + ": " + g))
        sv = hf.state_views(st, D, C, var["amsgrad"])
        _same(w, r["w"], what + ": w")
        for g in ("m_w", "v_w") + (("vmax_w",) if var["amsgrad"] else ()):
            _same(sv[g], r["state"][g], what + ": " + g)
        assert not sv["m_b"].any() and not sv["v_b"].any()
        for g in hf.HEADER:
            assert int(sv[g]) == r["state"][g], (what, g, int(sv[g]), r["state"][g])
        ok = r64["ok"]
        assert np.array_equal(r["pred"][ok] == r["y"][ok], r64["pred"][ok] == r64["y"][ok]), what + ": the twin's and the float64 rule's `correct` differ"
        w_rule, st_rule = r["w"], r["state"]
    return worst


@pytest.mark.parametrize("D", mc.DS)
@pytest.mark.parametrize("B", mc.BS)
def test_twin_against_the_float32_rule(B, D):
    """z, w, the moments and the figures word for word; rx, rw, cosv, g, h and the row loss within one fp32 unit in the last place of
    the float64 value (measured over the 125 shapes: at most 0.5, the one rounding).  One test per (B, D): its five C."""
    worst = dict.fromkeys(ROUNDED, 0.0)
    for C in mc.CS:
        for g, v in run_twin_case((B, D, C)).items():
            worst[g] = max(worst[g], v)
    print("twin B %d D %d: worst fp32 units %s" % (B, D, ", ".join("%s %.3f" % kv for kv in worst.items())))


def test_the_large_gpu_shapes_have_no_knife_edge():
    """The two shapes only the GPU runs: the conditions on the float64 rule's first step (the later steps are checked on the device's
    own values there)."""
    for shape in mc.GPU_SHAPES[len(mc.CPU_SHAPES):]:
        var = mc.variation(shape)
        p = mc.problem(mc.case_seed(shape), *shape, var)
        xp = hf._rule_batch(p["x"].astype(np.float64), p["labels"].astype(np.int64), shape[2], p["rows"], shape[0], p["keep"], mc.keep_scale(var), False)[2]
        w = p["w"].astype(np.float64)
        rx, rw = 1.0 / np.sqrt((xp * xp).sum(axis=1)), 1.0 / np.sqrt((w * w).sum(axis=1))
        y = p["labels"][p["rows"]].astype(np.int64)
        for k in range(mc.STEPS):
            kw = mc.step_kw(var, k)
            det = hf.margin_logits_rule(xp @ w.T, rx, rw, y, kw["s"], kw["m"], kw["easy_margin"])
            mc.assert_no_knife_edge({"detail": det, "ok": np.ones(shape[0], bool), "y": y}, kw["easy_margin"], mc.case_id(shape))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the branches, declined rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("easy", (False, True))
def test_every_branch_is_entered_by_its_row(easy):
    p = mc.branch_problem()
    kw = dict(mc.BRANCH_KW, easy_margin=easy)
    r64 = hf.margin_step_rule(p["x"], p["labels"], p["w"].astype(np.float64), **kw)
    mc.assert_no_knife_edge(r64, easy, "branch rows")
    det = r64["detail"]
    assert det["theta_m"][0] > hf.MARGIN_CAP + 1e-4 and det["inside"][0, 0] and abs(det["cos"][0, 0]) < 1 - 1e-5       # capped, not clamped
    assert (det["dfac"][0, 0] == 0.0) == (not easy) and (easy or det["out"][0, 0] == math.cos(hf.MARGIN_CAP))
    assert det["cos"][1, 0] == 1.0 and not det["inside"][1, 0] and det["dfac"][1, 0] == 0.0 and r64["g"][1, 0] == 0.0  # clamped
    assert r64["rx"][2] == 1e12 and not det["cos"][2].any() and det["inside"][2].all()                                 # a zero-norm row
    assert r64["rw"][3] == 1e12 and not det["cos"][:, 3].any()                                                         # a zero centre
    assert (det["out"][2, 1] == 0.0) == easy                                            # easy margin passes an exact 0 through
    w = p["w"].copy()
    st = np.zeros(hf.margin_state_bytes(4, 4, True), np.uint8)
    v = hf.margin_workspace_views(hf.margin_step_host(p["x"], p["labels"], w, st, **kw), 6, 4)
    r = hf.margin_step_rule(p["x"], p["labels"], p["w"], dtype=F32, given={g: v[g].copy() for g in GIVEN}, **kw)
    assert v["rx"][2] == hf.MARGIN_RMAX and v["rw"][3] == hf.MARGIN_RMAX and v["cosv"][1, 0] == F32(hf.MARGIN_HI)
    assert v["g"][1, 0] == 0.0 and v["h"][1, 0] == 0.0 and (easy or (v["g"][0, 0] == 0.0 and v["h"][0, 0] == 0.0))
    exact = exact_halves(p["x"], p["labels"], p["w"], v, None, None, 1.0, dict(kw, clear=False))
    for g in ROUNDED:
        within_one_ulp(v[g], exact[g], "branch rows: " + g)
    _same(w, r["w"], "branch rows: w")
    # the zero centre has no projection term: its gradient is rw times the chain, and Adam moves it off zero
    assert np.array_equal(r["dw"][3], (hf.MARGIN_RMAX * hf.dot32(v["g"].T[3][None, :], p["x"].T)).astype(F32)) and w[3].any()
    np.testing.assert_allclose(r["dw"], r64["dw"], rtol=2e-5, atol=1e-6 * float(np.abs(r64["dw"]).max()))
    assert np.array_equal(r["pred"] == r["y"], r64["pred"] == r64["y"])


@pytest.mark.parametrize("shape", ((1, 4, 1), (5, 1, 3)), ids=("C1", "D1"))
def test_one_class_and_one_dimension(shape):
    """C = 1: p = 1 and every gradient is zero, the weights only decay.  D = 1: every cosine is +-1, the clamp stops every gradient."""
    var = mc.VARIATIONS[1]
    p = mc.problem(5, *shape, var)
    w, st = p["w"].copy(), np.zeros(hf.margin_state_bytes(shape[1], shape[2], True), np.uint8)
    v = hf.margin_workspace_views(_host_step(p, var, 2, w, st), shape[0], shape[2])
    assert not v["g"].any() and not v["h"].any() and np.isfinite(v["row_loss"]).all()
    if shape[1] == 1:
        assert (np.abs(v["cosv"]) == F32(hf.MARGIN_HI)).all()
    r = _rule_step(p, var, 2, p["w"], None, F32)
    _same(w, r["w"], "w")
    assert int(hf.state_views(st, shape[1], shape[2], True)["t"]) == 1


@pytest.mark.parametrize("kind", mc.BAD_KINDS)
def test_a_declined_row_counts_for_nothing(kind):
    """A declined row inserted into a batch: the weights, the state and every other row's workspace are the bits of the batch without
    it; its own row is +0 in z, cosv, g and h, +0 in rx, NaN in the loss, -1 in row_src."""
    shape, at = (33, 65, 18), 7
    var = mc.variation(shape)
    p = mc.problem(mc.case_seed(shape), *shape, var)
    q = mc.with_bad_row(p, kind, at)
    B, D, C = shape
    out = []
    for prob, nb in ((p, B), (q, B + 1)):
        w, st = prob["w"].copy(), np.zeros(hf.margin_state_bytes(D, C, var["amsgrad"]), np.uint8)
        for k in range(2):
            ws = _host_step(prob, var, k, w, st)
        out.append((w, st, hf.margin_workspace_views(ws, nb, C)))
    (w0, st0, v0), (w1, st1, v1) = out
    _same(w0, w1, kind + ": w")
    _same(st0, st1, kind + ": state")
    others = np.arange(B + 1) != at
    for g in ("z", "cosv", "g", "h", "row_loss", "rx", "row_src"):
        _same(v0[g], v1[g][others], kind + ": " + g)
        assert np.isnan(v1[g][at]) if g == "row_loss" else (v1[g][at] == -1 if g == "row_src" else not np.any(v1[g][at])), (kind, g)
    assert not np.signbit(v1["g"][at]).any() and not np.signbit(v1["rx"][at])
    _same(v0["rw"], v1["rw"], kind + ": rw")


def test_a_nan_centre_reaches_every_row_the_target_included():
    """The logits are not screened (the linear step's stance): a NaN in w_3 makes column 3 of z NaN and with it every row's softmax -
    also the rows whose target is class 3, where a NaN theta + m is NOT taken for a capped one (torch.minimum keeps a NaN too)."""
    shape = (33, 65, 18)
    var = mc.VARIATIONS[1]
    p = mc.problem(11, *shape, var)
    p["labels"][p["rows"][:4]] = 3
    w = p["w"].copy()
    w[3, 2] = np.nan
    st = np.zeros(hf.margin_state_bytes(65, 18, True), np.uint8)
    for k in (0, 1):
        st_k = st.copy()
        v = hf.margin_workspace_views(_host_step(p, var, k, w.copy(), st_k), 33, 18)
        assert np.isnan(v["z"][:, 3]).all() and np.isnan(v["rw"][3]) and np.isnan(v["g"]).all() and np.isnan(v["row_loss"]).all(), k
        r = _rule_step(p, var, k, w, None, F32)
        assert np.isnan(r["g"]).all() and np.isnan(r["row_loss"]).all()
        # (the arg-max passes over a NaN logit on both sides: a row whose target is class 3 is never correct)
        assert r["state"]["correct"] == int(hf.state_views(st_k, 65, 18, True)["correct"]) <= 29


def test_an_all_declined_batch_changes_nothing_but_the_workspace():
    shape = (33, 65, 18)
    var = mc.VARIATIONS[1]
    p = mc.problem(9, *shape, var)
    w, st = p["w"].copy(), np.zeros(hf.margin_state_bytes(65, 18, True), np.uint8)
    _host_step(p, var, 0, w, st)
    w1, st1 = w.copy(), st.copy()
    p["rows"] = np.where(np.arange(33) % 2 == 0, -1, p["N"]).astype(np.int32)
    ws = np.full(hf.margin_workspace_bytes(*shape), 0xFF, np.uint8)
    v = hf.margin_workspace_views(_host_step(p, var, 1, w, st, ws, clear=False), 33, 18)
    _same(w, w1, "w")
    sv, sv1 = hf.state_views(st, 65, 18, True), hf.state_views(st1, 65, 18, True)
    assert int(sv["n"]) == 0 and int(sv["t"]) == 1 == int(sv1["t"])
    for g in sv:
        if g != "n":
            _same(sv[g], sv1[g], g)
    assert not v["z"].any() and not v["g"].any() and not v["h"].any() and not v["cosv"].any() and not v["rx"].any()
    assert np.isnan(v["row_loss"]).all() and (v["row_src"] == -1).all() and (v["rw"] > 0).all()
    r = hf.margin_step_rule(p["x"], p["labels"], w1, None, rows=p["rows"], dtype=F32, s=5.0, m=0.3)
    assert r["n"] == 0 and r["state"]["t"] == 0 and np.array_equal(r["w"], w1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_margin_entry_points_are_declared_bound_and_element_aligned():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_head_fit_margin_state_bytes", 3), ("frmap_head_fit_margin_workspace_bytes", 3),
                       ("frmap_head_fit_margin_step", 22), ("frmap_head_fit_margin_step_host", 22)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10          # only symbols are added
    rows = _lib.ALIGNMENT["frmap_head_fit_margin_step"]
    assert list(rows) == ["x", "labels", "rows", "keep", "w", "state", "workspace"]
    assert all(cls == "element" for cls, _ in rows.values())
    assert [n for _, n in rows.values()] == [4, 4, 4, 1, 4, 8, 4]
    # ... as the header states them
    doc = header[header.index("Head fitting with a margin"):header.index("size_t frmap_head_fit_margin_state_bytes")]
    assert "x, labels, rows, w and workspace need their element size (4), keep 1, state the size\n * of a uint64 counter (8)" in doc
    assert "frmap_head_fit_margin_step_host" not in _lib.ALIGNMENT
    assert {"frmap_head_fit_margin_state_bytes", "frmap_head_fit_margin_workspace_bytes"} <= set(oc.pointer_free())
    for name in ("margin_state_bytes", "margin_workspace_bytes", "margin_workspace_views", "margin_step", "margin_step_host",
                 "margin_step_rule", "margin_schedule", "MarginHead", "fit_margin_head"):
        assert callable(getattr(hf, name)), name


def test_margin_sizes():
    lib = _lib.load()
    for D, C in ((1, 1), (3, 2), (512, 1000), (65, 33)):
        for ams in (0, 1):
            assert lib.frmap_head_fit_margin_state_bytes(D, C, ams) == lib.frmap_head_fit_state_bytes(D, C, ams) == hf.margin_state_bytes(D, C, bool(ams))
        for B in (1, 32, 33):
            assert lib.frmap_head_fit_margin_workspace_bytes(B, D, C) == 4 * (4 * B * C + 3 * B + C) == hf.margin_workspace_bytes(B, D, C)
            v = hf.margin_workspace_views(np.zeros(hf.margin_workspace_bytes(B, D, C), np.uint8), B, C)
            assert v["z"].shape == v["cosv"].shape == v["g"].shape == v["h"].shape == (B, C)
            assert v["row_loss"].shape == v["rx"].shape == v["row_src"].shape == (B,) and v["rw"].shape == (C,)
    for bad in ((0, 1), (1, 0), (65537, 1), (1, 65537)):
        assert lib.frmap_head_fit_margin_state_bytes(*bad, 0) == 0 and lib.frmap_head_fit_margin_workspace_bytes(4, *bad) == 0, bad
    assert lib.frmap_head_fit_margin_workspace_bytes(0, 2, 2) == 0 and lib.frmap_head_fit_margin_workspace_bytes(2 ** 20 + 1, 2, 2) == 0
    assert lib.frmap_head_fit_margin_workspace_bytes(2 ** 20, 2, 65536) == 4 * (4 * 2 ** 36 + 3 * 2 ** 20 + 65536)
    with pytest.raises(ValueError, match="C = 0"):
        hf.margin_state_bytes(2, 0)
    with pytest.raises(ValueError, match="B = 0"):
        hf.margin_workspace_bytes(0, 2, 2)


def test_twin_and_launcher_refusals_name_the_argument():
    """Both come before anything is read, written or launched: host dummy pointers serve."""
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.uint8)
    p = (buf.ctypes.data + 255) // 256 * 256
    ok = dict(x=p, labels=p, rows=0, keep=0, ks=1.0, w=p, state=p, workspace=p, N=1, B=1, D=1, C=1, flags=0)
    floats = (9.6, 0.45, 0.05, 1e-3, 0.9, 0.999, 1e-8, 0.0)

    def args(**kw):
        a = dict(ok, **kw)
        return [a[k] for k in ("x", "labels", "rows", "keep", "ks", "w", "state", "workspace", "N", "B", "D", "C")] + list(floats) + [a["flags"]]
    refused = [(dict(flags=8), "flags"), (dict(flags=32), "flags"), (dict(N=0), "N"), (dict(B=0), "B"), (dict(B=2 ** 20 + 1), "B"), (dict(D=0), "D"),
               (dict(D=65537), "D"), (dict(C=0), "C"), (dict(C=65537), "C"), (dict(N=0, B=0), "N"), (dict(B=0, D=0), "B"), (dict(D=0, C=0), "D"),
               (dict(C=0, flags=8), "C"), (dict(flags=8, w=0), "flags"), (dict(x=0), "null pointer"), (dict(labels=0), "null pointer"),
               (dict(w=0), "null pointer"), (dict(state=0), "null pointer"), (dict(workspace=0), "null pointer")]
    for kw, word in refused:
        for name, fn, last in (("head_fit_margin_step_host", lib.frmap_head_fit_margin_step_host, 0), ("head_fit_margin_step", lib.frmap_head_fit_margin_step, None)):
            assert fn(*args(**kw), last) == -1, (name, kw)
            msg = lib.frmap_last_error().decode()
            assert msg.startswith(name + ": ") and oc.names_operand(msg, word.split()[0]), (name, kw, msg)
            assert msg[len(name) + 2:].startswith(word), (name, kw, msg)            # the FIRST failing check of the shared order
    assert lib.frmap_head_fit_margin_step(*args(flags=8), None) == -1 and "16 easy margin" in lib.frmap_last_error().decode()
    for arg, need in (("x", 4), ("labels", 4), ("rows", 4), ("w", 4), ("state", 8), ("workspace", 4)):
        assert lib.frmap_head_fit_margin_step(*args(**{arg: p + need // 2}), None) == -1, arg
        msg = lib.frmap_last_error().decode()
        assert msg.startswith("head_fit_margin_step: ") and "%s must be %d-byte aligned" % (arg, need) in msg, (arg, msg)
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
    N, B, D, C = 9, 4, 8, 6
    g = torch.Generator().manual_seed(1)
    return dict(x=torch.randn((N, D), generator=g), labels=torch.tensor([0, 1, 2, 3, 4, 5, 0, 1, 2], dtype=torch.int32), w=torch.randn((C, D), generator=g),
                state=torch.zeros((hf.margin_state_bytes(D, C, amsgrad),), dtype=torch.uint8),
                workspace=torch.zeros((hf.margin_workspace_bytes(B, D, C),), dtype=torch.uint8), rows=torch.tensor([0, 3, 8, -1], dtype=torch.int32),
                keep=torch.ones((B, D), dtype=torch.uint8))


ORDER = ("x", "labels", "w", "state", "workspace", "rows", "keep")
# the axes along which an operand's extent is another operand's (x gives N and D, w's first axis C, rows B)
DEPENDENT = {"labels": (0,), "w": (1,), "state": (0,), "workspace": (0,), "keep": (0, 1)}


def _call(values, **kw):
    return hf.margin_step(*[_gpu(values[k]) for k in ORDER], 1.0, **dict(dict(s=9.6, m=0.45), **kw))


def test_the_valid_margin_call_reaches_the_library(stub):
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(_valid())
    assert e.value.entry == "frmap_head_fit_margin_step" and e.value.args_[8:12] == (9, 4, 8, 6) and e.value.args_[20] == 0
    assert e.value.args_[12:15] == (9.6, 0.45, 0.0) and len(stub.calls) == 1
    v = _valid(True)
    v["keep"] = v["rows"] = None
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(v, amsgrad=True, clear=True, decoupled=True, easy_margin=True, label_smoothing=0.05, batch=4)
    assert e.value.args_[2] == 0 and e.value.args_[3] == 0 and e.value.args_[20] == 23 and e.value.args_[14] == 0.05


@pytest.mark.parametrize("operand", sorted(DEPENDENT))
def test_a_dependent_margin_operand_is_refused_before_the_library(operand, stub):
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
        hf.margin_step(*[values[k] if k == operand else _gpu(values[k]) for k in ORDER], 1.0, s=9.6, m=0.45)
    assert oc.names_operand(str(e.value), operand)
    assert stub.calls == []


def test_free_margin_operands_are_refused(stub):
    for operand, bad, exc in (("x", torch.zeros((9,)), ValueError), ("x", torch.zeros((9, 8), dtype=torch.float64), TypeError),
                              ("rows", torch.zeros((2, 2), dtype=torch.int32), ValueError), ("rows", torch.zeros((4,), dtype=torch.int64), TypeError),
                              ("w", None, TypeError)):
        values = _valid()
        values[operand] = bad
        with pytest.raises(exc):
            _call(values)
    with pytest.raises(ValueError, match="state"):                    # the AMSGrad state is larger
        _call(_valid(), amsgrad=True)
    with pytest.raises(ValueError):
        hf.MarginHead(8, 0, "cpu")
    with pytest.raises(ValueError):
        hf.MarginHead(hf.MAX_D + 1, 4, "cpu")
    assert stub.calls == []


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. MarginHead
# ---------------------------------------------------------------------------------------------------------------------------------
def test_margin_head_initialises_as_the_reference_and_loads_into_an_arcface_net():
    import frmap_amd
    D, C = 512, 7
    head = hf.MarginHead(D, C, "cpu", amsgrad=True, generator=torch.Generator().manual_seed(7))
    torch.manual_seed(7)
    ref = torch.empty(C, D)
    torch.nn.init.xavier_normal_(ref, gain=math.sqrt(2))
    assert torch.equal(head.weight, ref)
    assert head.state.numel() == hf.margin_state_bytes(D, C, True) and not head.state.any()
    fig = head.epoch_figures()
    assert fig["rows"] == 0 and fig["t"] == 0 and np.isnan(fig["accuracy"])
    assert sorted(head.state_dict()) == ["weight"]
    model = frmap_amd.get_model("arcface", C)
    head.load_into(model)
    assert torch.equal(model.arcface.weight.detach(), head.weight)
    with pytest.raises(ValueError, match=re.escape("arcface.weight is [7, 512], the head is [9, 512]")):
        hf.MarginHead(D, 9, "cpu").load_into(model)
    with pytest.raises(ValueError, match="the head is"):
        hf.MarginHead(256, C, "cpu").load_into(model)
    for other in ("baseline", "siamese"):
        with pytest.raises(ValueError, match="an ArcFaceNet expected"):
            head.load_into(frmap_amd.get_model(other, C))
    with pytest.raises(ValueError, match="an ArcFaceNet expected"):
        head.load_into(torch.nn.Linear(D, C))


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the synthetic fit with the float32 rule
# ---------------------------------------------------------------------------------------------------------------------------------
FIT_START, FIT_END = 0.16796875, 0.82421875


def test_the_float32_rule_learns_the_synthetic_classes():
    """`fit_margin_cases.FIT` at its pinned seed through the reference's schedule (an epoch every 4 steps), AdamW, AMSGrad, smoothing
    0.05: the validation accuracy by the largest cosine is 0.16796875 (43 / 256) with the initial centres and 0.82421875 (211 / 256)
    after 60 steps of the float32 rule.  Asserted: the start exactly (it is data), the end at 0.80 or better."""
    f = mc.FIT
    xt, yt, xv, yv, w, steps = mc.fit_data()
    start = mc.cosine_accuracy(w, xv, yv)
    st = None
    for k, rows in enumerate(steps):
        m_eff, s_eff = hf.margin_schedule(k // f["steps_per_epoch"])
        r = hf.margin_step_rule(xt, yt, w, st, rows=rows, s=s_eff, m=m_eff, lr=f["lr"], label_smoothing=0.05, decoupled=True, amsgrad=True,
                                weight_decay=1e-4, dtype=F32)
        w, st = r["w"], r["state"]
    end = mc.cosine_accuracy(w, xv, yv)
    print("synthetic fit, float32 rule: validation accuracy %.8f -> %.8f, train accuracy under the margin %.3f" % (start, end, st["correct"] / st["rows"]))
    assert st["t"] == f["steps"] and st["rows"] == f["steps"] * f["batch"]
    assert start == FIT_START and end >= 0.80, (start, end)


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the check program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_margin_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/head_fit_margin_check.cpp (its own `main`, head_fit_twin.h, the two rule headers and tools/head_fit_check_common.h, nothing
    else) built with -fsanitize=address,undefined (runtimes linked statically) and run directly as a child process: it sweeps shapes of
    `fit_margin_cases` with every buffer a heap block of exactly its size, and exits 0."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "head_fit_margin_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    src_path = os.path.join(ROOT, "tools", "head_fit_margin_check.cpp")
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc, src_path, "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.stdout.splitlines()[-2:] == ["16 cases", "self check passed"], run.stdout[-500:]
    src = open(src_path).read()                                                  # the program's shapes are of this module's table
    shapes = [tuple(int(v) for v in s) for s in re.findall(r"\{(\d+), (\d+), (\d+)\}", src[src.index("shapes[][3]"):src.index("long cases")])]
    assert len(shapes) == 8 and set(shapes) <= set(mc.CPU_SHAPES)
