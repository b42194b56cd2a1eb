"""CPU: head fitting in groups - the C ABI of the five new entry points, the group's host twin (`head_fit.group_step_host`) against
H runs of the single host twin on head h's slices word for word over `fit_group_cases`, the head whose rows are all declined, flag 8
(evaluate only), the refusals of the twin and - under `operand_cases`' stub, nothing launches - of `head_fit.group_step`,
`kfold_rows` against sklearn's `KFold`, and tools/head_fit_group_check.cpp under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fit_group_cases as gc
import operand_cases as oc
from frmap_amd import _lib, head_fit as hf, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CASES = gc.cases()


def _same(a, b, what):
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d bytes differ, first at byte %d" % (what, bad.size, int(bad[0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_group_entry_points_are_declared_bound_and_element_aligned():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_head_fit_group_state_stride", 3), ("frmap_head_fit_group_state_bytes", 4),
                       ("frmap_head_fit_group_workspace_bytes", 4), ("frmap_head_fit_group_step", 16), ("frmap_head_fit_group_step_host", 16)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10
    rows = _lib.ALIGNMENT["frmap_head_fit_group_step"]
    assert list(rows) == ["x", "labels", "rows", "keep", "hyper", "w", "b", "state", "workspace"]
    assert all(cls == "element" for cls, _ in rows.values())
    assert [n for _, n in rows.values()] == [4, 4, 4, 1, 4, 4, 4, 8, 4]
    assert "frmap_head_fit_group_step_host" not in _lib.ALIGNMENT
    assert {"frmap_head_fit_group_state_stride", "frmap_head_fit_group_state_bytes", "frmap_head_fit_group_workspace_bytes"} <= set(oc.pointer_free())
    assert not hasattr(ops, "head_fit_group_step") and oc.census()
    for name in ("group_state_stride", "group_state_bytes", "group_workspace_bytes", "group_step", "group_step_host", "group_step_rule",
                 "HeadGroup", "kfold_rows", "cross_validate", "sweep_heads"):
        assert callable(getattr(hf, name)), name


def test_group_sizes():
    """The stride is the single size rounded up to a multiple of 8.  `frmap_head_fit_state_bytes` itself already reports a multiple
    of 8, so the two are equal; what the stride is strictly larger than, for (D, C) = (2, 1) with AMSGrad, is the state's CONTENT -
    64 + 12 x (C D + C) = 100 bytes, no multiple of 8 - and it equals the content where that is one (no AMSGrad)."""
    lib = _lib.load()
    for D, C in ((2, 1), (1, 1), (3, 2), (512, 18), (65, 33)):
        for ams in (0, 1):
            single = lib.frmap_head_fit_state_bytes(D, C, ams)
            content = 64 + 4 * (C * D + C) * (3 if ams else 2)
            stride = lib.frmap_head_fit_group_state_stride(D, C, ams)
            assert stride == (single + 7) // 8 * 8 == (content + 7) // 8 * 8 == hf.group_state_stride(D, C, bool(ams))
            assert lib.frmap_head_fit_group_state_bytes(5, D, C, ams) == 5 * stride
            if not ams:
                assert stride == content
    assert hf.group_state_stride(2, 1, True) == 104 > 64 + 12 * 3 and hf.group_state_stride(2, 1, False) == 64 + 8 * 3
    assert lib.frmap_head_fit_group_workspace_bytes(5, 32, 512, 18) == 5 * lib.frmap_head_fit_workspace_bytes(32, 512, 18) > 0
    for bad in ((0, 2, 1, 0), (4097, 2, 1, 0), (1, 0, 1, 0), (1, 1, 65537, 0)):
        assert lib.frmap_head_fit_group_state_bytes(*bad) == 0, bad
    assert lib.frmap_head_fit_group_state_bytes(4096, 2, 1, 0) == 4096 * 88
    assert lib.frmap_head_fit_group_workspace_bytes(0, 4, 2, 1) == 0 and lib.frmap_head_fit_group_workspace_bytes(4097, 4, 2, 1) == 0
    assert lib.frmap_head_fit_group_workspace_bytes(2, 0, 2, 1) == 0 and lib.frmap_head_fit_group_state_stride(0, 1, 0) == 0
    with pytest.raises(ValueError, match="H = 0"):
        hf.group_state_bytes(0, 2, 1)
    t = hf.hyper_table(3, lr=[1, 2, 3], weight_decay=0.5, keep_scale=[1.0, 2.0, 4.0])
    assert t.shape == (3, 8) and t.dtype == F32 and t[:, 0].tolist() == [1, 2, 3] and t[:, 4].tolist() == [0.5] * 3
    assert t[:, 6].tolist() == [1, 2, 4] and not t[:, 7].any() and t[0, 1] == F32(0.9)
    with pytest.raises(ValueError, match="lr"):
        hf.hyper_table(3, lr=[1, 2])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2., 3. the twin against H single twins
# ---------------------------------------------------------------------------------------------------------------------------------
def _fresh_states(H, D, C, amsgrad, fill):
    """Zeroed state contents `stride` apart, the padding bytes between them at `fill`."""
    stride, content = hf.group_state_stride(D, C, amsgrad), 64 + 4 * (C * D + C) * (3 if amsgrad else 2)
    st = np.full((H * stride,), fill, np.uint8)
    for h in range(H):
        st[h * stride: h * stride + content] = 0
    return st, stride, content


@pytest.mark.parametrize("case", CASES, ids=[gc.case_id(c) for c in CASES])
def test_group_twin_equals_single_twins_on_the_slices(case):
    """Every word of w, b, the state and the workspace at each of three steps, under the fills 0xFF and 0x5A of the padding bytes
    (which stay untouched) and of the fresh workspace; the all-declined head of the `DEAD` cases keeps w, b, moments and t."""
    H, B, D, C, var = case
    x, labels, w0, b0, rows, keep = gc.problem(1000 + CASES.index(case), H, B, D, C, var["keep"], var["dead"])
    work = hf.workspace_bytes(B, D, C)
    for fill in (0xFF, 0x5A):
        w, b = w0.copy(), b0.copy()
        st, stride, content = _fresh_states(H, D, C, var["amsgrad"], fill)
        ws = np.full((H * work,), fill, np.uint8)
        singles = [(w0[h].copy(), b0[h].copy(), np.zeros(hf.state_bytes(D, C, var["amsgrad"]), np.uint8)) for h in range(H)]
        for s in range(gc.STEPS):
            table = gc.hyper(H, var["keep"], s)
            hf.group_step_host(x, labels, rows, table, w, b, st, ws, keep, decoupled=var["decoupled"], amsgrad=var["amsgrad"], clear=s == 0)
            for h in range(H):
                wh, bh, sh = singles[h]
                wsh = hf.step_host(x, labels, wh, bh, sh, None, rows[h], None if keep is None else keep[h], float(table[h, 6]),
                                   **gc.single_kw(table, h, var, clear=s == 0))
                gw, gb, _, _, gs, gws = gc.slices(h, H, B, D, C, var["amsgrad"], w, b, rows, keep, st, ws)
                what = "%s fill 0x%02X step %d head %d" % (gc.case_id(case), fill, s, h)
                _same(gw, wh, what + ": w")
                _same(gb, bh, what + ": b")
                _same(gs[:content], sh[:content], what + ": state")
                _same(gws, wsh, what + ": workspace")
                assert (st[h * stride + content: (h + 1) * stride] == fill).all(), what + ": padding bytes written"
        for h in range(H):
            sv = hf.state_views(st[h * stride: h * stride + hf.state_bytes(D, C, var["amsgrad"])].copy(), D, C, var["amsgrad"])
            if h == var["dead"]:
                assert int(sv["t"]) == 0 and int(sv["n"]) == 0 and int(sv["rows"]) == 0
                _same(w[h], w0[h], "the all-declined head: w")
                _same(b[h], b0[h], "the all-declined head: b")
                assert not any(sv[k].any() for k in sv if sv[k].shape), "the all-declined head: moments"
            else:
                assert int(sv["t"]) == gc.STEPS and int(sv["n"]) >= 1 and int(sv["rows"]) == gc.STEPS * int(sv["n"])
                assert not np.array_equal(w[h], w0[h])
    assert any(c[4]["dead"] is not None and c[0] > 1 for c in CASES)


def test_group_rule_is_h_single_rules():
    """`group_step_rule` (float32 mode, on the twin's own z, g and row losses) gives the twin's words; its evaluate mode keeps w, b, t."""
    H, B, D, C = 2, 7, 5, 3
    var = {"keep": True, "decoupled": False, "amsgrad": True, "dead": None}
    x, labels, w, b, rows, keep = gc.problem(5, H, B, D, C, True)
    table = gc.hyper(H, True)
    st, stride, content = _fresh_states(H, D, C, True, 0)
    wt, bt = w.copy(), b.copy()
    ws = hf.group_step_host(x, labels, rows, table, wt, bt, st, None, keep, amsgrad=True, clear=True)
    work = hf.workspace_bytes(B, D, C)
    given = [{k: v for k, v in hf.workspace_views(ws[h * work: (h + 1) * work], B, C).items() if k != "row_src"} for h in range(H)]
    out = hf.group_step_rule(x, labels, w, b, None, rows, keep, hyper=table, amsgrad=True, clear=True, dtype=F32, given=given)
    for h in range(H):
        _same(out[h]["w"], wt[h], "rule w")
        _same(out[h]["b"], bt[h], "rule b")
        sv = hf.state_views(st[h * stride: h * stride + hf.state_bytes(D, C, True)].copy(), D, C, True)
        for name in sv:
            if sv[name].shape:
                _same(out[h]["state"][name], sv[name], name)
            else:
                assert int(sv[name]) == out[h]["state"][name], name
    ev = hf.group_step_rule(x, labels, w, b, None, rows, None, hyper=table, amsgrad=True, evaluate=True, dtype=F32)
    for h in range(H):
        assert np.array_equal(ev[h]["w"], w[h]) and ev[h]["state"]["t"] == 0 and ev[h]["state"]["rows"] == ev[h]["n"] >= 1
        assert not ev[h]["state"]["m_w"].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. flag 8
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[1] in (5, 33)], ids=[gc.case_id(c) for c in CASES if c[1] in (5, 33)])
def test_evaluate_only_on_the_twin(case):
    H, B, D, C, var = case
    ams = var["amsgrad"]
    x, labels, w, b, rows, keep = gc.problem(77, H, B, D, C, False, var["dead"])
    table = gc.hyper(H, False)
    st, stride, content = _fresh_states(H, D, C, ams, 0x5A)
    kw = dict(decoupled=var["decoupled"], amsgrad=ams)
    hf.group_step_host(x, labels, rows, table, w, b, st, None, None, clear=True, **kw)              # one training step: t = 1, moments set
    w1, b1, st1 = w.copy(), b.copy(), st.copy()
    ws_e = hf.group_step_host(x, labels, rows, table, w, b, st, None, None, evaluate=True, **kw)    # adds to the step's figures
    wc, bc, stc = w1.copy(), b1.copy(), st1.copy()
    ws_t = hf.group_step_host(x, labels, rows, table, wc, bc, stc, None, None, **kw)                # a training step on a copy
    _same(w, w1, "evaluate: w")
    _same(b, b1, "evaluate: b")
    _same(ws_e, ws_t, "evaluate: the workspace is the training step's")
    for h in range(H):
        e, o, t = (a[h * stride: (h + 1) * stride] for a in (st, st1, stc))
        _same(e[40:], o[40:], "evaluate: reserved words, moments and padding of head %d" % h)
        eh, oh, th = e[:40].view(np.uint64), o[:40].view(np.uint64), t[:40].view(np.uint64)
        assert eh[0] == oh[0] and (eh[0] == 1 or h == var["dead"]), "t is not advanced"
        assert eh[1:5].tolist() == th[1:5].tolist(), (h, eh.tolist(), th.tolist())
        assert eh[2] == 2 * oh[2] and (th[0] == oh[0] + 1 or h == var["dead"])
    # flag 4 with flag 8 clears first; two calls accumulate
    hf.group_step_host(x, labels, rows, table, w, b, st, None, None, evaluate=True, clear=True, **kw)
    once = [st[h * stride: h * stride + 40].view(np.uint64).copy() for h in range(H)]
    hf.group_step_host(x, labels, rows, table, w, b, st, None, None, evaluate=True, **kw)
    for h in range(H):
        twice = st[h * stride: h * stride + 40].view(np.uint64)
        assert once[h][2] == once[h][1] and twice[2:5].tolist() == (2 * once[h][2:5]).tolist() and twice[0] == once[h][0]
    _same(w, w1, "three evaluate calls: w")
    with pytest.raises(ValueError, match="keep"):
        hf.group_step_host(x, labels, rows, table, w, b, st, None, np.ones((H, B, D), np.uint8), evaluate=True, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_twin_and_launcher_refusals_name_the_argument():
    """Both come before anything is read, written or launched: host dummy pointers serve."""
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.uint8)
    p = (buf.ctypes.data + 255) // 256 * 256
    ok = dict(x=p, labels=p, rows=p, keep=0, hyper=p, w=p, b=p, state=p, workspace=p, N=1, H=1, B=1, D=1, C=1, flags=0)

    def args(**kw):
        a = dict(ok, **kw)
        return [a[k] for k in ("x", "labels", "rows", "keep", "hyper", "w", "b", "state", "workspace", "N", "H", "B", "D", "C", "flags")]
    refused = [(dict(H=0), "H"), (dict(H=4097), "H"), (dict(flags=16), "flags"), (dict(rows=0), "rows"), (dict(hyper=0), "hyper"),
               (dict(keep=p, flags=8), "keep"), (dict(N=0), "N"), (dict(B=0), "B"), (dict(B=2 ** 20 + 1), "B"), (dict(D=65537), "D"),
               (dict(C=0), "C"), (dict(w=0), "null pointer")]
    for kw, word in refused:
        for name, fn, last in (("head_fit_group_step_host", lib.frmap_head_fit_group_step_host, 0), ("head_fit_group_step", lib.frmap_head_fit_group_step, None)):
            assert fn(*args(**kw), last) == -1, (name, kw)
            msg = lib.frmap_last_error().decode()
            assert msg.startswith(name + ": ") and oc.names_operand(msg, word.split()[0]), (name, kw, msg)
    for kw, word in ((dict(x=p + 2), "x must be 4-byte aligned"), (dict(rows=p + 1), "rows must be 4-byte aligned"),
                     (dict(hyper=p + 2), "hyper must be 4-byte aligned"), (dict(state=p + 4), "state must be 8-byte aligned"),
                     (dict(workspace=p + 2), "workspace must be 4-byte aligned"), (dict(b=p + 1), "b must be 4-byte aligned")):
        assert lib.frmap_head_fit_group_step(*args(**kw), None) == -1, kw
        msg = lib.frmap_last_error().decode()
        assert msg.startswith("head_fit_group_step: ") and word in msg, (kw, msg)
    assert not buf.any()
    # the single step still refuses bit 8
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)
    assert lib.frmap_head_fit_step(p, p, 0, 0, 1.0, p, p, p, p, 1, 1, 1, 1, *hyper, 8, None) == -1 and "flags = 8" in lib.frmap_last_error().decode()


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
    N, H, B, D, C = 9, 3, 4, 8, 2
    g = torch.Generator().manual_seed(1)
    return dict(x=torch.randn((N, D), generator=g), labels=torch.zeros((N,), dtype=torch.int32),
                rows=torch.tensor([[0, 3, 8, 1], [2, 2, -1, -1], [5, 6, 7, -1]], dtype=torch.int32),
                hyper=torch.from_numpy(hf.hyper_table(H, lr=1e-3)), w=torch.randn((H, C, D), generator=g), b=torch.zeros((H, C)),
                state=torch.zeros((hf.group_state_bytes(H, D, C, amsgrad),), dtype=torch.uint8),
                workspace=torch.zeros((hf.group_workspace_bytes(H, B, D, C),), dtype=torch.uint8), keep=torch.ones((H, B, D), dtype=torch.uint8))


ORDER = ("x", "labels", "rows", "hyper", "w", "b", "state", "workspace", "keep")
# the axes along which an operand's extent is another operand's (w's first two axes and rows' second GIVE H, C and B)
DEPENDENT = {"labels": (0,), "rows": (0,), "hyper": (0, 1), "w": (2,), "b": (0, 1), "state": (0,), "workspace": (0,), "keep": (0, 1, 2)}


def _call(values, **kw):
    return hf.group_step(*[_gpu(values[k]) for k in ORDER], **kw)


def test_the_valid_group_call_reaches_the_library(stub):
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(_valid())
    assert e.value.entry == "frmap_head_fit_group_step" and e.value.args_[9:15] == (9, 3, 4, 8, 2, 0) and len(stub.calls) == 1
    v = _valid(True)
    v["keep"] = None
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(v, amsgrad=True, clear=True, evaluate=True, decoupled=True)
    assert e.value.args_[3] == 0 and e.value.args_[14] == 15


@pytest.mark.parametrize("operand", sorted(DEPENDENT))
def test_a_dependent_group_operand_is_refused_before_the_library(operand, stub):
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
    args = [values[k].clone() if k == operand else _gpu(values[k]) for k in ORDER]          # this one stays a CPU tensor
    with pytest.raises(RuntimeError) as e:
        hf.group_step(*args)
    assert oc.names_operand(str(e.value), operand)
    assert stub.calls == []


def test_free_group_operands_and_flag_8_are_refused(stub):
    for operand, bad, exc in (("x", torch.zeros((9,)), ValueError), ("x", torch.zeros((9, 8), dtype=torch.float64), TypeError),
                              ("rows", None, ValueError), ("hyper", None, TypeError), ("w", None, ValueError)):
        values = _valid()
        values[operand] = bad
        with pytest.raises(exc):
            _call(values)
    with pytest.raises(ValueError, match="keep"):
        _call(_valid(), evaluate=True)
    with pytest.raises(ValueError, match="state"):                    # the AMSGrad state is larger
        _call(_valid(), amsgrad=True)
    with pytest.raises(ValueError):
        hf.HeadGroup(0, 8, 3, "cpu")
    with pytest.raises(ValueError):
        hf.HeadGroup(hf.MAX_H + 1, 8, 3, "cpu")
    assert stub.calls == []


def test_head_group_initialises_like_consecutive_linear_heads():
    gen = torch.Generator().manual_seed(7)
    group = hf.HeadGroup(3, 16, 4, "cpu", amsgrad=True, generator=gen)
    gen = torch.Generator().manual_seed(7)
    for h in range(3):
        one = hf.LinearHead(16, 4, "cpu", amsgrad=True, generator=gen)
        assert torch.equal(group.weight[h], one.weight) and torch.equal(group.bias[h], one.bias)
        view = group.head(h)
        assert view.weight.data_ptr() == group.weight[h].data_ptr() and view.state.numel() == hf.state_bytes(16, 4, True)
        assert view.state.data_ptr() == group.state.data_ptr() + h * group.stride and view.as_classifier()[1].data_ptr() == group.bias[h].data_ptr()
        assert sorted(view.state_dict()) == ["bias", "weight"]
    shared = hf.HeadGroup(3, 16, 4, "cpu", generator=torch.Generator().manual_seed(7), shared_init=True)
    assert all(torch.equal(shared.weight[h], group.weight[0]) and torch.equal(shared.bias[h], group.bias[0]) for h in range(3))
    assert group.state.numel() == 3 * group.stride and not group.state.any() and group.hyper.shape == (3, 8)
    figs = group.epoch_figures()
    assert len(figs) == 3 and all(f["rows"] == 0 and f["t"] == 0 and np.isnan(f["accuracy"]) for f in figs)
    with pytest.raises(IndexError):
        group.head(3)
    # the table is written only when a value changed
    table = hf.hyper_table(3, lr=[1, 2, 3])
    group.set_hyper(table)
    assert group.hyper[:, 0].tolist() == [1, 2, 3]
    group.hyper.zero_()                                 # (behind the group's back: an unchanged table is not copied again)
    group.set_hyper(table.copy())
    assert not group.hyper.any()
    group.set_hyper(hf.hyper_table(3, lr=[1, 2, 4]))
    assert group.hyper[:, 0].tolist() == [1, 2, 4]


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the folds
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 10, 11, 103])
@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("seed", [0, 42])
def test_kfold_rows_is_sklearns_kfold(N, k, seed):
    from sklearn.model_selection import KFold
    want = list(KFold(k, shuffle=True, random_state=seed).split(range(N)))
    got = hf.kfold_rows(N, k, seed)
    assert len(got) == len(want) == k
    for (tr, va), (wtr, wva) in zip(got, want):
        assert tr.dtype == va.dtype == np.int32 and np.array_equal(tr, wtr) and np.array_equal(va, wva)
        assert (np.diff(tr) > 0).all() and (np.diff(va) > 0).all() and len(tr) + len(va) == N
    with pytest.raises(ValueError):
        hf.kfold_rows(3, 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the check program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_group_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/head_fit_group_check.cpp (its own `main`, head_fit_twin.h, the two rule headers and tools/head_fit_check_common.h, nothing else) built with
    -fsanitize=address,undefined (runtimes linked statically) and run directly as a child process: it sweeps the table of
    `fit_group_cases` with every buffer a heap block of exactly its size, and exits 0."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "head_fit_group_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    src_path = os.path.join(ROOT, "tools", "head_fit_group_check.cpp")
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc, src_path, "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    assert run.stdout.splitlines()[-2:] == ["%d cases" % len(CASES), "self check passed"], run.stdout[-500:]
    src = open(src_path).read()                                                  # the program's table is this module's
    assert "Hs[] = {%s}" % ", ".join(str(h) for h in gc.HEADS) in src
    assert "shapes[][3] = {%s}" % ", ".join("{%d, %d, %d}" % s for s in gc.SHAPES) in src
