"""CPU: the embedding head-fitting step - a first step worked by hand, the float64 rule (`head_fit.embed_step_rule`) against torch
autograd through ``F.linear`` -> ``nn.BatchNorm1d`` in training mode -> the mask -> the reference's margin call sequence ->
``cross_entropy`` -> one Adam / AdamW over the four tensors for 25 steps, the host twin (`head_fit.embed_step_host`) against the
float32 rule over the shape table of `fit_embed_cases` (where the knife-edge conditions of every table are asserted too), the margin
half against `head_fit.margin_step_host`, declined rows, the all-or-nothing cases, a constant column, a dropped column, the C ABI of
the four entry points, the refusals of `head_fit.embed_step` under `operand_cases`' stub (nothing launches), `EmbedHead` and its
`load_into`, the synthetic fit with the float32 rule, and tools/head_fit_embed_check.cpp under the address and undefined-behaviour
sanitizers."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fit_embed_cases as ec
import fit_margin_cases as mc
import operand_cases as oc
from frmap_amd import _lib, head_fit as hf
from test_head_fit_margin_cpu import _torch_logits, within_one_ulp, _same, _Cuda, SAN_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MARGIN_GIVEN = ("z", "rx", "rw", "cosv", "g", "h", "row_loss")
STAGE1, STAGE3 = ("mean32", "rstd", "uvar", "ah"), ("da",)
EXACT = ("a", "yp", "gy", "dbeta", "dgamma", "lab", "row_src1", "n1")            # word for word between the twin and the float32 rule


def _host_step(p, var, k, params, st, ws=None, given=0, clear=None, **over):
    kw = dict(ec.step_kw(var, k, clear), **over)
    return hf.embed_step_host(p["x"], p["labels"], *[params[n] for n in ec.PARAMS], st, ws, rows=p["rows"], keep=p["keep"],
                              keep_scale=ec.keep_scale(var) if p["keep"] is not None else 1.0, given=given, **kw)


def _rule_step(p, var, k, params, state, dtype, clear=None, given=None, **over):
    kw = dict(ec.step_kw(var, k, clear), **over)
    return hf.embed_step_rule(p["x"], p["labels"], *[params[n] for n in ec.PARAMS], state, rows=p["rows"], keep=p["keep"],
                              keep_scale=ec.keep_scale(var) if p["keep"] is not None else 1.0, dtype=dtype, given=given, **kw)


def _fresh(p, amsgrad):
    return np.zeros(hf.embed_state_bytes(p["D"], p["E"], p["C"], amsgrad), np.uint8)


def exact_stages(p, v, params, kw, n1):
    """The float64 value of every rounded quantity of the BatchNorm stages FROM THE INPUTS IT IS ROUNDED FROM: the statistics from the
    fp32 ``a`` of the workspace views ``v``, ah from ``a``, ``mean32`` and ``rstd``, da from ``gy``, ``ah``, ``rstd``, ``dbeta``, ``dgamma``
    and the gamma of before the step."""
    ok = v["row_src1"] >= 0
    a = v["a"].astype(np.float64)
    mean = a[ok].sum(axis=0) / n1
    var = ((a[ok] - mean) ** 2).sum(axis=0) / n1
    out = {"mean32": mean, "rstd": 1.0 / np.sqrt(var + float(F32(kw["bn_eps"]))), "uvar": var * n1 / (n1 - 1)}
    out["ah"] = np.where(ok[:, None], (a - v["mean32"].astype(np.float64)) * v["rstd"].astype(np.float64), 0.0)
    g64 = params["gamma"].astype(np.float64) * v["rstd"].astype(np.float64)
    out["da"] = np.where(ok[:, None], g64 * ((v["gy"].astype(np.float64) - v["dbeta"].astype(np.float64) / n1)
                                             - v["ah"].astype(np.float64) * (v["dgamma"].astype(np.float64) / n1)), 0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. a first step by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_first_step_by_hand():
    """B = 2, D = 1, E = 1, C = 2, no mask, s = 2, m = 0, plain Adam with lr = 0.5.  x = (1, 3), w1 = 2: a = (2, 6); mean 4, var 4, so
    ah = -+1 / sqrt(1 + eps / 4) = -+r; gamma = 1, beta = 0.5: y' = 0.5 -+ r.  One dimension: every cosine is +-1 and clamped, so no
    gradient passes the margin stage: gy = 0, dbeta = dgamma = 0, da = 0, and Adam with a zero gradient moves no parameter by more than
    its zero first moment: w1, gamma, beta and wc stay.  The running statistics move: rm = 0.9 x 0 + 0.1 x 4 = 0.4, rv = 0.9 x 1 + 0.1 x 8
    = 1.7 (the unbiased variance of (2, 6) is 8).  t = 1 in the three headers, rows = 2."""
    x, labels = np.array([[1.0], [3.0]], F32), np.array([0, 1], np.int32)
    params = {"w1": np.array([[2.0]], F32), "gamma": np.ones(1, F32), "beta": np.full(1, 0.5, F32), "running_mean": np.zeros(1, F32),
              "running_var": np.ones(1, F32), "wc": np.array([[1.0], [-1.0]], F32)}
    kw = dict(bn_eps=1e-5, bn_momentum=0.1, s=2.0, m=0.0, lr=0.5)
    r = hf.embed_step_rule(x, labels, *[params[n] for n in ec.PARAMS], **kw)
    rr = 1.0 / math.sqrt(1.0 + 1e-5 / 4.0)
    assert r["taken"] and r["n1"] == 2 and r["n2"] == 2
    np.testing.assert_allclose(r["a"], [[2.0], [6.0]], rtol=0, atol=0)
    np.testing.assert_allclose(r["mean32"], [4.0], rtol=1e-15)
    np.testing.assert_allclose(r["rstd"], [1.0 / math.sqrt(4.0 + 1e-5)], rtol=1e-15)
    np.testing.assert_allclose(r["uvar"], [8.0], rtol=1e-15)
    np.testing.assert_allclose(r["ah"], [[-rr], [rr]], rtol=1e-15)
    np.testing.assert_allclose(r["yp"], [[0.5 - rr], [0.5 + rr]], rtol=1e-15)
    np.testing.assert_allclose(r["margin"]["detail"]["cs"], [[-(1 - 1e-7), 1 - 1e-7], [1 - 1e-7, -(1 - 1e-7)]], rtol=1e-15)
    assert not r["gy"].any() and not r["da"].any() and not r["dbeta"].any() and not r["dgamma"].any()
    for k in ("w1", "gamma", "beta", "wc"):
        np.testing.assert_array_equal(r[k], params[k].astype(np.float64))
    np.testing.assert_allclose(r["running_mean"], [0.4], rtol=1e-15)
    np.testing.assert_allclose(r["running_var"], [1.7], rtol=1e-15)
    assert [r["state"][k]["t"] for k in ("linear", "bn", "margin")] == [1, 1, 1] and r["state"]["margin"]["rows"] == 2
    # the same through the host twin, in float32
    st = np.zeros(hf.embed_state_bytes(1, 1, 2), np.uint8)
    p32 = {k: v.copy() for k, v in params.items()}
    hf.embed_step_host(x, labels, *[p32[n] for n in ec.PARAMS], st, **kw)
    for k in ("w1", "gamma", "beta", "wc"):
        np.testing.assert_array_equal(p32[k], params[k])
    assert p32["running_mean"][0] == F32(F32(0.1) * F32(4.0)) and abs(float(p32["running_var"][0]) - 1.7) < 1e-6
    views = hf.embed_state_views(st, 1, 1, 2)
    assert [int(views[k]["t"]) for k in ("linear", "bn", "margin")] == [1, 1, 1] and int(views["margin"]["rows"]) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the float64 rule against torch
# ---------------------------------------------------------------------------------------------------------------------------------
TORCH_CASES = (
    dict(shape=(6, 8, 7, 5), decoupled=False, amsgrad=False, ls=0.0, keep=False, easy=False),
    dict(shape=(33, 65, 34, 18), decoupled=True, amsgrad=True, ls=0.05, keep=True, easy=False),
    dict(shape=(16, 3, 4, 2), decoupled=True, amsgrad=False, ls=0.05, keep=False, easy=True),
    dict(shape=(9, 130, 12, 33), decoupled=False, amsgrad=True, ls=0.0, keep=True, easy=True),
)
TORCH_TOL = 1e-12


@pytest.mark.parametrize("case", TORCH_CASES, ids=["-".join(map(str, c["shape"])) + ("-easy" if c["easy"] else "") for c in TORCH_CASES])
def test_float64_rule_against_torch_over_25_steps(case):
    """Loss, the four parameters and both running statistics agree with torch's float64 autograd and optimiser to 1e-12 over 25 steps,
    with the schedule's scale and margin changing every step, a fresh batch and (where the case has one) a fresh mask per step."""
    B, D, E, C = case["shape"]
    rng = np.random.default_rng(177 + B)
    N = B + 4
    x = rng.standard_normal((N, D))
    labels = rng.integers(0, C, N)
    params = {"w1": rng.standard_normal((E, D)) / math.sqrt(D), "gamma": 1.0 + 0.1 * rng.standard_normal(E), "beta": 0.1 * rng.standard_normal(E),
              "running_mean": np.zeros(E), "running_var": np.ones(E), "wc": rng.standard_normal((C, E)) * math.sqrt(4.0 / (C + E))}
    lin = torch.nn.Linear(D, E, bias=False, dtype=torch.float64)
    bn = torch.nn.BatchNorm1d(E, eps=1e-5, momentum=0.1, dtype=torch.float64).train()
    wct = torch.tensor(params["wc"], dtype=torch.float64, requires_grad=True)
    with torch.no_grad():
        lin.weight.copy_(torch.tensor(params["w1"]))
        bn.weight.copy_(torch.tensor(params["gamma"]))
        bn.bias.copy_(torch.tensor(params["beta"]))
    tensors = {"w1": lin.weight, "gamma": bn.weight, "beta": bn.bias, "wc": wct}
    opt = (torch.optim.AdamW if case["decoupled"] else torch.optim.Adam)(list(tensors.values()), lr=1e-2, weight_decay=1e-2, amsgrad=case["amsgrad"])
    st, worst, worst_grad = None, 0.0, 0.0
    for k in range(25):
        m_eff, s_eff = hf.margin_schedule(k // 2, 32.0, 0.5)
        rows = rng.permutation(N)[:B]
        keep = (rng.random((B, E)) >= 0.25).astype(np.uint8) if case["keep"] else None
        scale = 1.0 / 0.75 if case["keep"] else 1.0
        for g in opt.param_groups:
            g["lr"] = mc.LRS[k % 3]
        y = bn(lin(torch.tensor(x[rows], dtype=torch.float64)))
        if keep is not None:
            y = y * torch.tensor(keep * scale, dtype=torch.float64)
        lab = torch.tensor(labels[rows])
        loss = F.cross_entropy(_torch_logits(y, wct, lab, s_eff, m_eff, case["easy"]), lab, label_smoothing=case["ls"])
        opt.zero_grad()
        loss.backward()
        r = hf.embed_step_rule(x, labels, *[params[n] for n in ec.PARAMS], st, rows=rows, keep=keep, keep_scale=scale, s=s_eff, m=m_eff,
                               easy_margin=case["easy"], lr=mc.LRS[k % 3], weight_decay=1e-2, label_smoothing=case["ls"],
                               decoupled=case["decoupled"], amsgrad=case["amsgrad"])
        assert r["taken"]
        ec.assert_norms(r, "step %d" % k)
        gt = lin.weight.grad.numpy()
        worst_grad = max(worst_grad, float(np.abs(r["dw1"] - gt).max() / max(np.abs(gt).max(), 1e-300)))
        assert abs(r["loss"] - float(loss.detach())) <= TORCH_TOL * max(1.0, abs(float(loss.detach()))), (k, r["loss"], float(loss.detach()))
        opt.step()
        params, st = {n: r[n] for n in ec.PARAMS}, r["state"]
        want = {**{n: t.detach().numpy() for n, t in tensors.items()}, "running_mean": bn.running_mean.numpy(), "running_var": bn.running_var.numpy()}
        for n in ec.PARAMS:
            worst = max(worst, float(np.abs(params[n] - want[n]).max()))
            np.testing.assert_allclose(params[n], want[n], rtol=TORCH_TOL, atol=TORCH_TOL, err_msg="%s, step %d" % (n, k))
    print("float64 rule against torch, %s: worst absolute difference of a parameter or statistic %.3g, worst relative dw1 difference %.3g"
          % (case["shape"], worst, worst_grad))
    assert st["margin"]["t"] == 25 and int(bn.num_batches_tracked) == 25


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the twin against the float32 rule
# ---------------------------------------------------------------------------------------------------------------------------------
def run_twin_case(shape, steps=ec.STEPS):
    """`steps` steps of the twin on a shape of the table, each checked against the float32 rule: the float64 stages within one fp32
    unit of the float64 value from their own inputs, everything else word for word against the rule given the twin's stage outputs.
    Returns the worst distance of a float64 stage, in units in the last place."""
    B, D, E, C = shape
    var = ec.variation(shape)
    p = ec.problem(ec.case_seed(shape), B, D, E, C, var)
    params, st, state = ec.params_of(p), _fresh(p, var["amsgrad"]), None
    worst = 0.0
    for k in range(steps):
        before = {n: v.copy() for n, v in params.items()}
        ws = _host_step(p, var, k, params, st)
        v = hf.embed_workspace_views(ws, B, E, C)
        kw = ec.step_kw(var, k)
        n1 = int(v["n1"][0])
        free = _rule_step(p, var, k, before, None, np.float64)                # the float64 rule on the same inputs: the knife edges
        mc.assert_no_knife_edge(free["margin"], kw["easy_margin"], "%s step %d" % (shape, k))
        ec.assert_norms(free, "%s step %d" % (shape, k))
        exact = exact_stages(p, v, before, kw, n1)
        for name in STAGE1 + STAGE3:
            worst = max(worst, within_one_ulp(v[name], exact[name], "%s step %d: %s" % (shape, k, name)))
        given = {**{n: v[n] for n in STAGE1 + STAGE3}, "margin": {n: v["margin"][n] for n in MARGIN_GIVEN}}
        r = _rule_step(p, var, k, before, state, F32, given=given)
        assert r["taken"] and r["n1"] == n1
        for name in EXACT:
            got = v[name][:1] if name == "n1" else v[name]
            want = np.array([r["n1"]], np.int32) if name == "n1" else np.asarray(r[name]).astype(got.dtype)
            _same(got, want, "%s step %d: %s" % (shape, k, name))
        for n in ec.PARAMS:
            _same(params[n], r[n].astype(F32), "%s step %d: %s" % (shape, k, n))
        views = hf.embed_state_views(st, D, E, C, var["amsgrad"])
        for part in ("linear", "bn", "margin"):
            for name, val in r["state"][part].items():
                got = views[part][name]
                if isinstance(val, np.ndarray):
                    _same(got, val.astype(F32), "%s step %d: state %s.%s" % (shape, k, part, name))
                else:
                    assert int(got) == val, (shape, k, part, name, int(got), val)
        state = r["state"]
    return worst


@pytest.mark.parametrize("shape", ec.SHAPES, ids=[ec.case_id(s) for s in ec.SHAPES])
def test_twin_against_the_float32_rule(shape):
    worst = run_twin_case(shape)
    print("twin against the float32 rule, %s: worst float64 stage %.3f units in the last place" % (ec.case_id(shape), worst))


def test_the_large_gpu_shapes_have_no_knife_edge():
    """The two one-step shapes of the GPU contract, on the float64 rule at the step the GPU test runs: the conditions of KNIFE EDGES hold."""
    for shape in ec.BIG_SHAPES:
        var = ec.variation(shape)
        p = ec.problem(ec.case_seed(shape), *shape, var)
        r = _rule_step(p, var, 2, ec.params_of(p), None, np.float64)
        assert r["taken"]
        mc.assert_no_knife_edge(r["margin"], ec.step_kw(var, 2)["easy_margin"], str(shape))
        ec.assert_norms(r, str(shape))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the margin half, declined rows, all or nothing, degenerate columns
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((33, 31, 33, 18), (5, 3, 1, 3)), ids=ec.case_id)
def test_the_margin_half_is_the_margin_twin_on_yp_and_lab(shape):
    """`margin_step_host` on the y' and lab of the workspace, the centres and the margin part of the state from before the step: its
    workspace, its centres and its state are the step's, bit for bit."""
    B, D, E, C = shape
    for var in ec.VARIATIONS:
        p = ec.problem(91, B, D, E, C, var)
        params, st = ec.params_of(p), _fresh(p, var["amsgrad"])
        for k in range(2):
            wc0 = params["wc"].copy()
            at, n = hf.embed_state_parts(D, E, C, var["amsgrad"])["margin"]
            st3 = st[at: at + n].copy()
            ws = _host_step(p, var, k, params, st)
            v = hf.embed_workspace_views(ws, B, E, C)
            kw = {a: b for a, b in ec.step_kw(var, k).items() if a not in ("bn_eps", "bn_momentum")}
            st3 = np.ascontiguousarray(st3)
            mws = hf.margin_step_host(v["yp"].copy(), v["lab"].copy(), wc0, st3, **kw)
            mv = hf.margin_workspace_views(mws, B, C)
            for name in MARGIN_GIVEN + ("row_src",):
                _same(v["margin"][name], mv[name], "step %d: %s" % (k, name))
            _same(params["wc"], wc0, "step %d: the centres" % k)
            _same(st[at: at + n], st3, "step %d: the margin state" % k)


@pytest.mark.parametrize("kind", mc.BAD_KINDS)
def test_a_declined_row_counts_for_nothing(kind):
    """A batch with a declined row inserted: parameters, statistics and state are those of the batch without it, and the workspace rows of
    the others are the same bytes."""
    shape = (33, 31, 33, 18)
    var = ec.VARIATIONS[0]
    p = ec.problem(55, *shape, var)
    q = ec.with_bad_row(p, kind, 7)
    out = []
    for prob in (p, q):
        params, st = ec.params_of(prob), _fresh(prob, var["amsgrad"])
        ws = _host_step(prob, var, 1, params, st, clear=True)
        out.append((params, st, hf.embed_workspace_views(ws, prob["B"], shape[2], shape[3])))
    (pa, sa, va), (pb, sb, vb) = out
    for n in ec.PARAMS:
        _same(pa[n], pb[n], n)
    _same(sa, sb, "the state")
    others = np.delete(np.arange(q["B"]), 7)
    for name in ("a", "ah", "yp", "gy", "da"):
        _same(va[name], vb[name][others], name)
        assert not vb[name][7].any(), name
    assert vb["row_src1"][7] == -1 and vb["lab"][7] == -1 and int(vb["n1"][0]) == p["B"]


def _untaken(p, var, params, st0=None):
    """One step that must not be taken, from a fresh state and from the state after a good step: every byte of the parameters and the
    state stays (word n of the three headers, the count of the step in flight, is 0 after it)."""
    D, E, C = p["D"], p["E"], p["C"]
    st = _fresh(p, var["amsgrad"]) if st0 is None else st0.copy()
    before_p, before_s = {n: v.copy() for n, v in params.items()}, st.copy()
    ws = _host_step(p, var, 1, params, st, clear=False)
    for n in ec.PARAMS:
        _same(params[n], before_p[n], n)
    views, was = hf.embed_state_views(st, D, E, C, var["amsgrad"]), hf.embed_state_views(before_s, D, E, C, var["amsgrad"])
    for part in views:
        assert int(views[part]["n"]) == 0, part
        was[part]["n"][...] = 0
    _same(st, before_s, "the state")
    return hf.embed_workspace_views(ws, p["B"], E, C)


@pytest.mark.parametrize("case", ("B1", "two of three declined", "nan in w1", "nan in gamma"))
def test_all_or_nothing(case):
    var = ec.VARIATIONS[1]
    B = 1 if case == "B1" else 3
    p = ec.problem(321, B, 5, 4, 3, var)
    good = ec.problem(321, 6, 5, 4, 3, var)
    params, st_good = ec.params_of(good), _fresh(good, var["amsgrad"])
    _host_step(good, var, 0, params, st_good)
    assert int(hf.embed_state_views(st_good, 5, 4, 3, var["amsgrad"])["margin"]["t"]) == 1
    if case == "two of three declined":
        p["rows"] = np.array([p["rows"][0], -1, p["N"]], np.int32)
    if case == "nan in w1":
        params["w1"][2, 1] = np.nan
    if case == "nan in gamma":
        params["gamma"][1] = np.nan
    for st0 in (None, st_good):
        v = _untaken(p, var, {n: t.copy() for n, t in params.items()}, st0)
        assert not v["da"].any()
        assert int(v["n1"][0]) == (1 if case in ("B1", "two of three declined") else 3)


def test_a_constant_column_and_a_dropped_column():
    """var = 0 in a column: rstd = 1 / sqrt(eps), ah = 0 there, y' = beta, finite everywhere, and the step is taken.  A keep column of
    zeros: y', gy and da of the column are +0, so w1's row and gamma / beta of the column see a zero gradient."""
    var = ec.VARIATIONS[0]
    p = ec.problem(77, 9, 4, 5, 3, var)
    p["x"][:, :] = np.round(p["x"] * 4) / 4
    params = ec.params_of(p)
    params["w1"][2] = 0.0                                               # column 2 of a is constant (zero)
    p["keep"][:, 3] = 0
    st = _fresh(p, var["amsgrad"])
    before = {n: v.copy() for n, v in params.items()}
    ws = _host_step(p, var, 0, params, st)
    v = hf.embed_workspace_views(ws, 9, 5, 3)
    assert int(hf.embed_state_views(st, 4, 5, 3)["margin"]["t"]) == 1
    assert v["rstd"][2] == F32(1.0 / math.sqrt(float(F32(1e-5)))) and not v["ah"][:, 2].any() and v["mean32"][2] == 0 and v["uvar"][2] == 0
    assert all(np.isfinite(v[k]).all() for k in ("ah", "yp", "gy", "da"))
    assert not v["yp"][:, 3].any() and not v["gy"][:, 3].any() and not v["da"][:, 3].any() and v["dbeta"][3] == 0 and v["dgamma"][3] == 0
    # coupled decay moves the dropped column's parameters by the decay alone: the same step with a zero gradient
    a = hf.adam_scalars32(1, ec.step_kw(var, 0)["lr"], 0.9, 0.999, 1e-8, var["weight_decay"])
    want = hf.adam32(a, np.zeros(1, F32), before["gamma"][3:4], np.zeros(1, F32), np.zeros(1, F32), None, var["decoupled"], False)[0]
    assert params["gamma"][3] == want[0]
    r = _rule_step(p, var, 0, before, None, F32, given={**{n: v[n] for n in STAGE1 + STAGE3}, "margin": {n: v["margin"][n] for n in MARGIN_GIVEN}})
    for n in ec.PARAMS:
        _same(params[n], r[n].astype(F32), n)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_embed_entry_points_are_declared_bound_and_element_aligned():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_head_fit_embed_state_bytes", 4), ("frmap_head_fit_embed_workspace_bytes", 4), ("frmap_head_fit_embed_step", 30),
                       ("frmap_head_fit_embed_step_host", 30)):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    rows = _lib.ALIGNMENT["frmap_head_fit_embed_step"]
    assert list(rows) == ["x", "labels", "rows", "keep", "w1", "gamma", "beta", "running_mean", "running_var", "wc", "state", "workspace"]
    assert rows["state"] == ("element", 8) and rows["keep"] == ("element", 1)
    assert all(rows[k] == ("element", 4) for k in rows if k not in ("state", "keep"))
    assert "frmap_head_fit_embed_step_host" not in _lib.ALIGNMENT and _lib.ABI_VERSION == 10


def test_embed_sizes_and_layout():
    lib = _lib.load()
    for D, E, C, ams in ((3, 1, 1, False), (512, 512, 18, True), (5, 7, 9, True)):
        parts = hf.embed_state_parts(D, E, C, ams)
        assert all(at % 8 == 0 and n % 8 == 0 for at, n in parts.values())
        assert parts["margin"][1] == hf.margin_state_bytes(E, C, ams)
        assert hf.embed_workspace_bytes(7, D, E, C) == 4 * (5 * 7 * E + 5 * E + 2 * 7 + 2) + hf.margin_workspace_bytes(7, E, C)
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (65537, 4, 4), (4, 65537, 4), (4, 4, 65537)):
        assert lib.frmap_head_fit_embed_state_bytes(*bad, 0) == 0 and lib.frmap_head_fit_embed_workspace_bytes(4, *bad) == 0
        with pytest.raises(ValueError):
            hf.embed_state_bytes(*bad)
    assert lib.frmap_head_fit_embed_workspace_bytes(0, 4, 4, 4) == 0 and lib.frmap_head_fit_embed_workspace_bytes((1 << 20) + 1, 4, 4, 4) == 0


def test_twin_and_launcher_refusals_name_the_argument():
    """The same text from the twin and from the launcher (whose refusals come before any HIP call: host dummies do)."""
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.uint8)
    at = (buf.ctypes.data + 255) // 256 * 256
    base = dict(N=9, B=4, D=3, E=2, C=5, flags=0)

    def call(entry, ptr=at, **over):
        a = dict(base, **over)
        tail = (0,) if entry.endswith("_host") else (None,)
        ptrs = [ptr if k == 4 else at for k in range(12)]
        args = ptrs[:4] + [1.0] + ptrs[4:] + [a["N"], a["B"], a["D"], a["E"], a["C"], 1e-5, 0.1, 9.6, 0.45, 0.0, 1e-2, 0.9, 0.999, 1e-8, 0.0, a["flags"]]
        rc = getattr(lib, entry)(*args, *(over.get("given", 0),) if entry.endswith("_host") else tail)
        return rc, lib.frmap_last_error().decode()
    for entry in ("frmap_head_fit_embed_step_host", "frmap_head_fit_embed_step"):
        for word, over in (("N is below 1", dict(N=0)), ("B is outside", dict(B=0)), ("D is outside", dict(D=65537)), ("C is outside", dict(C=0)),
                           ("E is outside", dict(E=0)), ("E is outside", dict(E=65537)), ("flags has unknown bits", dict(flags=8)),
                           ("16 easy margin", dict(flags=32)), ("null pointer", dict(ptr=None))):
            rc, msg = call(entry, **over)
            assert rc == -1 and word in msg and msg.startswith(entry[6:] + ": "), (entry, over, rc, msg)
    rc, msg = call("frmap_head_fit_embed_step_host", given=8)
    assert rc == -1 and "given has unknown bits" in msg
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the wrapper's refusals under the stub library
# ---------------------------------------------------------------------------------------------------------------------------------
def _gpu(t):
    return t.as_subclass(_Cuda) if isinstance(t, torch.Tensor) else t


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: None)
    monkeypatch.setattr(hf, "_stream", lambda: 0)
    return oc.install(monkeypatch)


def _valid(amsgrad=False):
    N, B, D, E, C = 9, 4, 8, 5, 6
    g = torch.Generator().manual_seed(1)
    vec = lambda: torch.randn((E,), generator=g)
    return dict(x=torch.randn((N, D), generator=g), labels=torch.tensor([0, 1, 2, 3, 4, 5, 0, 1, 2], dtype=torch.int32),
                w1=torch.randn((E, D), generator=g), gamma=vec(), beta=vec(), running_mean=vec(), running_var=vec().abs(),
                wc=torch.randn((C, E), generator=g), state=torch.zeros((hf.embed_state_bytes(D, E, C, amsgrad),), dtype=torch.uint8),
                workspace=torch.zeros((hf.embed_workspace_bytes(B, D, E, C),), dtype=torch.uint8),
                rows=torch.tensor([0, 3, 8, -1], dtype=torch.int32), keep=torch.ones((B, E), dtype=torch.uint8))


ORDER = ("x", "labels", "w1", "gamma", "beta", "running_mean", "running_var", "wc", "state", "workspace", "rows", "keep")
# the axes along which an operand's extent is another operand's (x gives N and D, w1's first axis E, wc's first axis C, rows B)
DEPENDENT = {"labels": (0,), "w1": (1,), "gamma": (0,), "beta": (0,), "running_mean": (0,), "running_var": (0,), "wc": (1,), "state": (0,),
             "workspace": (0,), "keep": (0, 1)}


def _call(values, **kw):
    return hf.embed_step(*[_gpu(values[k]) for k in ORDER], 1.0, **dict(dict(s=9.6, m=0.45), **kw))


def test_the_valid_embed_call_reaches_the_library(stub):
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(_valid())
    assert e.value.entry == "frmap_head_fit_embed_step" and e.value.args_[13:18] == (9, 4, 8, 5, 6) and e.value.args_[28] == 0
    assert e.value.args_[18:23] == (1e-5, 0.1, 9.6, 0.45, 0.0) and len(stub.calls) == 1
    v = _valid(True)
    v["keep"] = v["rows"] = None
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(v, amsgrad=True, clear=True, decoupled=True, easy_margin=True, label_smoothing=0.05, batch=4, bn_eps=1e-3, bn_momentum=0.2)
    assert e.value.args_[2] == 0 and e.value.args_[3] == 0 and e.value.args_[28] == 23 and e.value.args_[18:20] == (1e-3, 0.2)


@pytest.mark.parametrize("operand", sorted(DEPENDENT))
def test_a_dependent_embed_operand_is_refused_before_the_library(operand, stub):
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
        hf.embed_step(*[values[k] if k == operand else _gpu(values[k]) for k in ORDER], 1.0, s=9.6, m=0.45)
    assert oc.names_operand(str(e.value), operand)
    assert stub.calls == []


def test_free_embed_operands_are_refused(stub):
    for operand, bad, exc in (("x", torch.zeros((9,)), ValueError), ("x", torch.zeros((9, 8), dtype=torch.float64), TypeError),
                              ("rows", torch.zeros((2, 2), dtype=torch.int32), ValueError), ("rows", torch.zeros((4,), dtype=torch.int64), TypeError),
                              ("w1", None, TypeError), ("wc", None, TypeError)):
        values = _valid()
        values[operand] = bad
        with pytest.raises(exc):
            _call(values)
    with pytest.raises(ValueError, match="state"):                    # the AMSGrad state is larger
        _call(_valid(), amsgrad=True)
    with pytest.raises(ValueError):
        hf.EmbedHead(8, 0, 4, "cpu")
    with pytest.raises(ValueError):
        hf.EmbedHead(8, 4, hf.MAX_D + 1, "cpu")
    assert stub.calls == []


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. EmbedHead
# ---------------------------------------------------------------------------------------------------------------------------------
def test_embed_head_starts_from_the_model_and_loads_into_it():
    import frmap_amd
    C = 7
    model = frmap_amd.get_model("arcface", C)
    with torch.no_grad():
        model.bn.running_mean.normal_(0, 0.1)
        model.bn.weight.normal_(1, 0.1)
    head = hf.EmbedHead.from_model(model, "cpu", amsgrad=True)
    assert (head.D, head.E, head.C) == (512, 512, C) and head.bn_eps == model.bn.eps and head.bn_momentum == 0.1
    for name, t in head.state_dict().items():
        mod, attr = name.split(".")
        assert torch.equal(t, getattr(getattr(model, mod), attr).detach()) and t.data_ptr() != getattr(getattr(model, mod), attr).data_ptr(), name
    assert head.state.numel() == hf.embed_state_bytes(512, 512, C, True) and not head.state.any()
    assert head._header_at == hf.state_bytes(512, 512, True) + hf.state_bytes(1, 512, True)
    fig = head.epoch_figures()
    assert fig["rows"] == 0 and fig["t"] == 0 and np.isnan(fig["accuracy"])
    centres = head.centres()
    assert centres.weight.data_ptr() == head.wc.data_ptr() and centres.state.data_ptr() == head.state.data_ptr() + head._header_at
    assert (centres.D, centres.C) == (512, C) and centres.state.numel() == hf.margin_state_bytes(512, C, True)
    # a step count in the state: load_into advances num_batches_tracked by it, once
    head.state[head._header_at: head._header_at + 8].view(torch.int64)[0] = 5
    with torch.no_grad():
        head.w1.mul_(0.5)
        head.running_var.add_(1.0)
    was = int(model.bn.num_batches_tracked)
    head.load_into(model)
    for name, t in head.state_dict().items():
        mod, attr = name.split(".")
        assert torch.equal(t, getattr(getattr(model, mod), attr).detach()), name
    assert int(model.bn.num_batches_tracked) == was + 5
    head.load_into(model)
    assert int(model.bn.num_batches_tracked) == was + 5
    fresh = hf.EmbedHead(512, 512, 9, "cpu", generator=torch.Generator().manual_seed(3))
    assert torch.equal(fresh.gamma, torch.ones(512)) and torch.equal(fresh.running_var, torch.ones(512)) and not fresh.beta.any()
    with pytest.raises(ValueError, match=re.escape("arcface.weight is [7, 512], the head's is [9, 512]")):
        fresh.load_into(model)
    with pytest.raises(ValueError, match=re.escape("embedding.weight is [512, 512], the head's is [256, 512]")):
        hf.EmbedHead(512, 256, C, "cpu").load_into(model)
    for other in ("baseline", "siamese"):
        with pytest.raises(ValueError, match="an ArcFaceNet expected"):
            head.load_into(frmap_amd.get_model(other, C))
        with pytest.raises(ValueError, match="an ArcFaceNet expected"):
            hf.EmbedHead.from_model(frmap_amd.get_model(other, C), "cpu")
    with pytest.raises(ValueError, match="an ArcFaceNet expected"):
        head.load_into(torch.nn.Linear(512, C))
    with pytest.raises(ValueError, match="pooled"):
        hf.cache_features(frmap_amd.get_model("siamese", C), "cnn", [], layer="pooled")


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the synthetic fit with the float32 rule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_float32_rule_learns_the_synthetic_classes():
    """`fit_embed_cases.FIT` at its pinned seed through the reference's schedule (an epoch every 4 steps), AdamW, AMSGrad, smoothing 0.05,
    dropout 0.2 behind the BatchNorm: the validation accuracy of the DEPLOYED embedding (running statistics) by the largest cosine
    rises.  Asserted: the end is at 0.80 or better and above the start; both figures are printed and recorded in DESIGN.md."""
    f = ec.FIT
    xt, yt, xv, yv, params, steps = ec.fit_data()
    start = ec.deployed_accuracy(params, xv, yv)
    rng = np.random.default_rng(3)
    st = None
    for k, rows in enumerate(steps):
        m_eff, s_eff = hf.margin_schedule(k // f["steps_per_epoch"])
        keep = (rng.random((f["batch"], f["E"])) >= 0.2).astype(np.uint8)
        r = hf.embed_step_rule(xt, yt, *[params[n] for n in ec.PARAMS], st, rows=rows, keep=keep, keep_scale=1.25, s=s_eff, m=m_eff, lr=f["lr"],
                               label_smoothing=0.05, decoupled=True, amsgrad=True, weight_decay=1e-4, dtype=F32)
        assert r["taken"]
        params, st = {n: r[n] for n in ec.PARAMS}, r["state"]
    end = ec.deployed_accuracy(params, xv, yv)
    print("synthetic fit, float32 rule: validation accuracy of the deployed embedding %.8f -> %.8f" % (start, end))
    assert st["margin"]["t"] == f["steps"] and st["margin"]["rows"] == f["steps"] * f["batch"]
    assert end >= 0.80 and end > start, (start, end)


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the check program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_embed_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/head_fit_embed_check.cpp (its own `main`, head_fit_twin.h, the two rule headers and tools/head_fit_check_common.h, nothing
    else) built with -fsanitize=address,undefined (runtimes linked statically) and run directly as a child process: it sweeps shapes of
    `fit_embed_cases` with every buffer a heap block of exactly its size, and exits 0."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "head_fit_embed_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    src_path = os.path.join(ROOT, "tools", "head_fit_embed_check.cpp")
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc, src_path, "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.stdout.splitlines()[-2:] == ["16 cases", "self check passed"], run.stdout[-500:]
    src = open(src_path).read()                                                  # the program's shapes are of this module's table
    shapes = [tuple(int(v) for v in s) for s in re.findall(r"\{(\d+), (\d+), (\d+), (\d+)\}", src[src.index("shapes[][4]"):src.index("long cases")])]
    assert len(shapes) == 8 and all(s in ec.SHAPES for s in shapes), shapes
