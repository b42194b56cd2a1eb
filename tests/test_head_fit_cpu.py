"""CPU: head fitting - the rule in numpy (`head_fit.step_rule`) on a hand-built case with every number written out, the float64
rule against torch (``nn.Linear`` + ``F.cross_entropy`` + ``optim.Adam`` / ``AdamW``) over 25 steps, dropout masks, declined rows,
the kernels' host twin (`head_fit.step_host`: the header the kernels compile) against the float32-mode rule word for word over the
sweep of `fit_cases`, tools/head_fit_check.cpp under the address and undefined-behaviour sanitizers, the C ABI of the new entry
points with their alignment rows, and the operand refusals of `head_fit.step` under `operand_cases`' stub (nothing launches)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fit_cases as fc
import operand_cases as oc
from frmap_amd import _lib, head_fit as hf, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hand_built_first_step_every_number_written_out():
    """B = 3, D = 2, C = 2, zero weights: p = 1/2 everywhere, so every figure is a small fraction."""
    x = np.array([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]])
    y = np.array([0, 1, 0])
    r = hf.step_rule(x, y, np.zeros((2, 2)), np.zeros(2), lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8)
    assert r["n"] == 3 and np.array_equal(r["z"], np.zeros((3, 2))) and r["row_src"].tolist() == [0, 1, 2]
    assert np.allclose(r["row_loss"], np.log(2.0), atol=1e-15) and abs(r["loss"] - np.log(2.0)) < 1e-15
    g = np.array([[-1, 1], [1, -1], [-1, 1]]) / 6.0                       # (p - onehot) / 3
    assert np.allclose(r["g"], g, atol=1e-16)
    dw = np.array([[-2.0, 1.0], [2.0, -1.0]]) / 6.0                       # g^T x: class 0 = -(x0 + x2) / 6 + x1 / 6
    db = np.array([-1.0, 1.0]) / 6.0
    assert np.allclose(r["dw"], dw, atol=1e-16) and np.allclose(r["db"], db, atol=1e-16)
    # first Adam step: m = 0.1 grad, v = 0.001 grad^2, m / bc1 = grad, sqrt(v / bc2) = |grad|: every parameter moves by lr sign(grad)
    # (up to eps / |grad| ~ 1e-7 relative)
    assert np.allclose(r["w"], -0.1 * np.sign(dw), atol=1e-7) and np.allclose(r["b"], -0.1 * np.sign(db), atol=1e-7)
    assert np.allclose(r["state"]["m_w"], 0.1 * dw, atol=1e-16) and np.allclose(r["state"]["v_w"], 0.001 * dw * dw, atol=1e-16)
    st = r["state"]
    assert (st["t"], st["n"], st["rows"], st["correct"]) == (1, 3, 3, 2)            # ties: the first arg-max is class 0
    assert st["loss_q"] == 3 * int(np.rint(float(F32(np.log(2.0))) * 2 ** 24))
    # label smoothing 0.2: y = (0.9, 0.1), loss still log 2 (p uniform), g = (0.5 - 0.9, 0.5 - 0.1) / 3 for label 0
    r = hf.step_rule(x, y, np.zeros((2, 2)), np.zeros(2), lr=0.1, label_smoothing=0.2)
    assert np.allclose(r["g"][0], [-0.4 / 3, 0.4 / 3], atol=1e-16) and np.allclose(r["row_loss"], np.log(2.0), atol=1e-15)
    # the float32 mode of the same case
    r32 = hf.step_rule(x, y, np.zeros((2, 2)), np.zeros(2), lr=0.1, dtype=F32)
    assert r32["w"].dtype == F32 and np.allclose(r32["w"], -0.1 * np.sign(dw), atol=1e-6) and r32["state"]["correct"] == 2


def _torch_steps(x, y, w0, b0, batches, masks, ls, decoupled, amsgrad, lr, wd):
    lin = torch.nn.Linear(w0.shape[1], w0.shape[0]).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w0))
        lin.bias.copy_(torch.from_numpy(b0))
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(lin.parameters(), lr=lr, weight_decay=wd, amsgrad=amsgrad)
    out = []
    for rows, mask in zip(batches, masks):
        xb = torch.from_numpy(x[rows])
        if mask is not None:
            xb = xb * torch.from_numpy(mask.astype(np.float64)) * (1.0 / 0.9)
        opt.zero_grad()
        loss = F.cross_entropy(lin(xb), torch.from_numpy(y[rows]).long(), label_smoothing=ls)
        loss.backward()
        opt.step()
        out.append((float(loss), lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()))
    return out


@pytest.mark.parametrize("B,D,C,ls", [(32, 64, 18, 0.0), (33, 65, 5, 0.05), (7, 3, 2, 0.0), (64, 512, 36, 0.05)])
@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("dropout", [False, True])
def test_rule_against_torch_in_float64(B, D, C, ls, decoupled, amsgrad, dropout):
    """25 steps of fresh random batches; loss, weights and bias agree to 1e-12 (a numpy restatement of the formulas measured
    1.8e-15 against torch).  ``dropout``: the rule with `keep` against torch with the same mask applied by hand."""
    rng = np.random.default_rng(B * 1000 + D + int(decoupled) * 7 + int(amsgrad) * 13)
    N = 4 * B
    x, y = rng.standard_normal((N, D)), rng.integers(0, C, N)
    w, b = rng.standard_normal((C, D)) / np.sqrt(D), rng.standard_normal(C) * 0.1
    batches = [rng.permutation(N)[:B] for _ in range(25)]
    masks = [(rng.random((B, D)) >= 0.1).astype(np.uint8) if dropout else None for _ in range(25)]
    want = _torch_steps(x, y, w, b, batches, masks, ls, decoupled, amsgrad, 1e-2, 1e-2)
    st, worst = None, 0.0
    for k, (rows, mask) in enumerate(zip(batches, masks)):
        r = hf.step_rule(x, y, w, b, st, rows, mask, 1.0 / 0.9, lr=1e-2, weight_decay=1e-2, label_smoothing=ls, decoupled=decoupled,
                         amsgrad=amsgrad)
        w, b, st = r["w"], r["b"], r["state"]
        worst = max(worst, abs(r["loss"] - want[k][0]), float(np.abs(w - want[k][1]).max()), float(np.abs(b - want[k][2]).max()))
    print("rule against torch B=%d D=%d C=%d ls=%g decoupled=%s amsgrad=%s dropout=%s: worst difference %.3g" % (
        B, D, C, ls, decoupled, amsgrad, dropout, worst))
    assert worst <= 1e-12 and st["t"] == 25 and st["rows"] == 25 * B


def test_declined_rows_contribute_nothing():
    rng = np.random.default_rng(3)
    N, B, D, C = 40, 12, 6, 4
    x, y = rng.standard_normal((N, D)), rng.integers(0, C, N)
    w, b = rng.standard_normal((C, D)), rng.standard_normal(C)
    rows = rng.permutation(N)[:B]
    x[rows[2], 3], x[rows[5], 0], y[rows[7]], y[rows[8]] = np.nan, -np.inf, C, -1
    bad = rows.copy()
    bad[0], bad[10] = -1, N
    good = np.array([r for i, r in enumerate(bad) if i not in (0, 2, 5, 7, 8, 10)])
    kw = dict(lr=1e-2, weight_decay=1e-2, label_smoothing=0.05, amsgrad=True)
    a, c = hf.step_rule(x, y, w, b, None, bad, **kw), hf.step_rule(x, y, w, b, None, good, **kw)
    assert a["n"] == c["n"] == 6 and a["row_src"].tolist() == [-1, bad[1], -1, bad[3], bad[4], -1, bad[6], -1, -1, bad[9], -1, bad[11]]
    for name in ("w", "b", "dw", "db"):
        assert np.array_equal(a[name], c[name]), name                      # bit for bit in float64
    for name in ("m_w", "v_w", "m_b", "v_b", "vmax_w", "t", "rows", "correct", "loss_q"):
        assert np.array_equal(a["state"][name], c["state"][name]), name
    keep = np.delete(np.arange(B), (0, 2, 5, 7, 8, 10))
    assert np.array_equal(a["g"][keep], c["g"]) and not a["g"][[0, 2, 5, 7, 8, 10]].any() and np.isnan(a["row_loss"][[0, 2]]).all()
    # every row declined: weights, moments and t untouched
    st = a["state"]
    z = hf.step_rule(x, np.full(N, -1), a["w"], a["b"], st, rows, **kw)
    assert z["n"] == 0 and np.array_equal(z["w"], a["w"]) and np.array_equal(z["b"], a["b"]) and z["state"]["t"] == st["t"] == 1
    for name in ("m_w", "v_w", "m_b", "v_b", "vmax_w", "vmax_b", "rows", "correct", "loss_q"):
        assert np.array_equal(z["state"][name], st[name]), name
    assert np.isnan(z["loss"])


def test_fma32_is_correctly_rounded_where_the_double_sum_is_not():
    """a b + c whose float64 sum lands on a float32 tie: the plain double rounding goes to even, fmaf follows the sticky bits."""
    a, b = F32(1 + 2.0 ** -23), F32(1 + 2.0 ** -23)          # a b = 1 + 2^-22 + 2^-46 exactly
    c = F32(2.0 ** -24)                                       # the sum is 1 + 2^-22 + 2^-24 + 2^-46: just above a tie of 2^-23 steps
    naive = F32(np.float64(a) * np.float64(b) + np.float64(c))
    got = hf.fma32(a, b, c)
    assert got == F32(1 + 3 * 2.0 ** -23) and float(got) >= float(naive)
    big = F32(2.0 ** 30)                                      # a b + c where c swallows the product's tail in float64 too
    assert hf.fma32(F32(1 + 2.0 ** -23), F32(1 - 2.0 ** -23), -big) == F32(1.0 - 2.0 ** 30)
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(1000).astype(F32), rng.standard_normal(1000).astype(F32)
    assert np.array_equal(hf.fma32(x, y, F32(0)), (x.astype(np.float64) * y).astype(F32))     # one rounding of an exact product


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin against the float32-mode rule
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("B", fc.SWEEP_B)
def test_twin_equals_the_float32_rule_word_for_word(B):
    """z, w, b, m, v, vmax and the figures bit for bit; g and the row loss - where the C library's exp / log and numpy's may
    differ - within one float32 unit in the last place of the float64 value (both sides evaluate the softmax in float64 and round
    once, so they sit at half a unit), and everything downstream on the twin's own g."""
    for D in fc.SWEEP_D:
        for C in fc.SWEEP_C:
            idx = fc.shapes().index((B, D, C))
            var = fc.variation(idx)
            x, labels, w, b, rows, keep = fc.problem(100 + idx, B, D, C, True, var["rows"], var["keep"])
            kw = dict(fc.HYPER, label_smoothing=var["label_smoothing"], decoupled=var["decoupled"], amsgrad=var["amsgrad"])
            st = np.zeros((hf.state_bytes(D, C, var["amsgrad"]),), np.uint8)
            wt, bt, rst = w.copy(), b.copy(), None
            what = "B=%d D=%d C=%d %s" % (B, D, C, var)
            for s in range(fc.STEPS):
                ws = hf.step_host(x, labels, wt, bt, st, None, rows, keep, 1.0 / 0.75, clear=s == 0, batch=B, **kw)
                tw = hf.workspace_views(ws, B, C)
                own = hf.step_rule(x, labels, w, b, rst, rows, keep, 1.0 / 0.75, dtype=F32, clear=s == 0, batch=B, **kw)
                assert _bits_equal(own["z"], tw["z"]) and np.array_equal(own["row_src"], tw["row_src"]), what
                ok = tw["row_src"] >= 0
                n = int(ok.sum())
                if n:
                    g64, l64 = fc.softmax64(tw["z"][ok], labels[tw["row_src"][ok]], n, var["label_smoothing"], C)
                    for got in (tw, own):
                        assert (np.abs(got["g"][ok] - g64) <= fc.ulp32(g64)).all(), what
                        assert (np.abs(got["row_loss"][ok] - l64) <= fc.ulp32(l64)).all(), what
                # downstream of the twin's own z, g and row losses: every word
                r = hf.step_rule(x, labels, w, b, rst, rows, keep, 1.0 / 0.75, dtype=F32, clear=s == 0, batch=B,
                                 given={k: tw[k] for k in ("z", "g", "row_loss")}, **kw)
                sv = hf.state_views(st, D, C, var["amsgrad"])
                assert _bits_equal(r["w"], wt) and _bits_equal(r["b"], bt), what
                for name in sv:
                    if sv[name].shape:
                        assert _bits_equal(r["state"][name], sv[name]), (what, name)
                    else:
                        assert int(sv[name]) == r["state"][name], (what, name, int(sv[name]), r["state"][name])
                w, b, rst = r["w"], r["b"], r["state"]
            assert rst["t"] == fc.STEPS and rst["rows"] == fc.STEPS * rst["n"] and rst["n"] >= 1


def test_twin_refusals_and_sizes():
    lib = _lib.load()
    assert lib.frmap_head_fit_state_bytes(512, 18, 0) == 64 + 8 * (512 * 18 + 18) and lib.frmap_head_fit_state_bytes(512, 18, 1) == 64 + 12 * (512 * 18 + 18)
    assert lib.frmap_head_fit_state_bytes(1, 1, 0) == 80 and lib.frmap_head_fit_state_bytes(0, 1, 0) == 0 and lib.frmap_head_fit_state_bytes(1, 0, 0) == 0
    assert lib.frmap_head_fit_state_bytes(1, 65537, 0) == 0 and lib.frmap_head_fit_state_bytes(512, 10000, 1) > 0      # the limit is above 10 000
    assert lib.frmap_head_fit_workspace_bytes(32, 512, 18) == 4 * (2 * 32 * 18 + 2 * 32) == lib.frmap_head_fit_workspace_bytes(32, 1, 18)
    assert lib.frmap_head_fit_workspace_bytes(0, 512, 18) == 0 and lib.frmap_head_fit_workspace_bytes(2 ** 20 + 1, 512, 18) == 0
    assert hf.state_layout(3, 2, True)["vmax_b"] == (64 + 4 * (6 + 6 + 2 + 2 + 6), np.float32, (2,))
    x, y = np.zeros((4, 3), F32), np.zeros(4, np.int32)
    w, b = np.zeros((2, 3), F32), np.zeros(2, F32)
    st = np.zeros(hf.state_bytes(3, 2), np.uint8)
    with pytest.raises(ValueError, match="keep"):
        hf.step_host(x, y, w, b, st, keep=np.ones((4, 2), np.uint8))
    with pytest.raises(ValueError, match="state"):
        hf.step_host(x, y, w, b, st[:-8])
    with pytest.raises(ValueError, match="workspace"):
        hf.step_host(x, y, w, b, st, np.zeros(hf.workspace_bytes(4, 3, 2) + 4, np.uint8))
    with pytest.raises(ValueError, match="exceed"):
        hf.step_host(x, y, w, b, st, batch=5)
    assert not st.any() and not w.any()
    # the launcher's refusals come before any HIP call: host dummy pointers serve (and nothing is written)
    buf = np.zeros(4096, np.uint8)
    p = (buf.ctypes.data + 255) // 256 * 256
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)
    for args, word in (((p, p, 0, 0, 1.0, p, p, p, p, 0, 1, 1, 1, *hyper, 0), "N = 0"), ((p, p, 0, 0, 1.0, p, p, p, p, 1, 0, 1, 1, *hyper, 0), "B = 0"),
                       ((p, p, 0, 0, 1.0, p, p, p, p, 1, 1, 0, 1, *hyper, 0), "D = 0"), ((p, p, 0, 0, 1.0, p, p, p, p, 1, 1, 1, 0, *hyper, 0), "C = 0"),
                       ((p, p, 0, 0, 1.0, p, p, p, p, 1, 1, 1, 65537, *hyper, 0), "C = 65537"),
                       ((p, p, 0, 0, 1.0, p, p, p, p, 1, 1, 1, 1, *hyper, 8), "flags = 8"),
                       ((p + 2, p, 0, 0, 1.0, p, p, p, p, 1, 1, 1, 1, *hyper, 0), "x must be 4-byte aligned"),
                       ((p, p, p + 1, 0, 1.0, p, p, p, p, 1, 1, 1, 1, *hyper, 0), "rows must be 4-byte aligned"),
                       ((p, p, 0, 0, 1.0, p, p, p + 4, p, 1, 1, 1, 1, *hyper, 0), "state must be 8-byte aligned"),
                       ((p, p, 0, 0, 1.0, p, p, p, p + 2, 1, 1, 1, 1, *hyper, 0), "workspace must be 4-byte aligned"),
                       ((p, p, 0, 0, 1.0, p, 0, p, p, 1, 1, 1, 1, *hyper, 0), "null pointer")):
        assert lib.frmap_head_fit_step(*args, None) == -1, word
        msg = lib.frmap_last_error().decode()
        assert msg.startswith("head_fit_step: ") and word in msg, (word, msg)
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the check program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/head_fit_check.cpp (its own `main`, head_fit_twin.h, the two rule headers and tools/head_fit_check_common.h, nothing else) built with
    -fsanitize=address,undefined (runtimes linked statically) and run directly: it sweeps the grid of `fit_cases` with every buffer a
    heap block of exactly its size, and exits 0."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "head_fit_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc,
                            os.path.join(ROOT, "tools", "head_fit_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    n = len(fc.SWEEP_B) * len(fc.SWEEP_D) * len(fc.SWEEP_C)
    assert run.stdout.splitlines()[-2:] == ["%d cases" % n, "self check passed"], run.stdout[-500:]
    src = open(os.path.join(ROOT, "tools", "head_fit_check.cpp")).read()
    for name, grid in (("Bs", fc.SWEEP_B), ("Ds", fc.SWEEP_D), ("Cs", fc.SWEEP_C)):          # the program's grid is this module's
        assert "%s[] = {%s}" % (name, ", ".join(str(v) for v in grid)) in src, name


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_head_fit_entry_points_are_declared_bound_and_element_aligned():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_head_fit_state_bytes", 3), ("frmap_head_fit_workspace_bytes", 3), ("frmap_head_fit_step", 21),
                       ("frmap_head_fit_step_host", 21)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10
    rows = _lib.ALIGNMENT["frmap_head_fit_step"]
    assert list(rows) == ["x", "labels", "rows", "keep", "w", "b", "state", "workspace"]
    assert all(cls == "element" for cls, _ in rows.values())
    assert {a: n for a, (_, n) in rows.items()} == {"x": 4, "labels": 4, "rows": 4, "keep": 1, "w": 4, "b": 4, "state": 8, "workspace": 4}
    for name in ("frmap_head_fit_step_host", "frmap_head_fit_state_bytes", "frmap_head_fit_workspace_bytes"):
        assert name not in _lib.ALIGNMENT
    assert {"frmap_head_fit_state_bytes", "frmap_head_fit_workspace_bytes"} <= set(oc.pointer_free())
    build = open(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", "build.sh")).read()
    assert " head_fit.hip " in build
    for h in ("head_fit_rule.h", "head_fit_twin.h"):
        assert os.path.isfile(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", h))
    rule = open(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", "head_fit_rule.h")).read()
    assert "FRMAP_HEAD_FIT_CHAIN = %d;" % hf.CHAIN in rule and "FRMAP_HEAD_FIT_MAX_C = %d;" % hf.MAX_C in rule and hf.MAX_C >= 10000
    # the tensor-taking wrappers live in `head_fit`, not among the public callables of `ops` (operand_cases' census pins that set)
    assert not hasattr(ops, "head_fit_step") and oc.census()
    for name in ("step_rule", "step", "step_host", "LinearHead", "cache_features", "fit_head"):
        assert callable(getattr(hf, name))
    with pytest.raises(ValueError, match="siamese"):
        hf.fit_head(None, "siamese", [])
    with pytest.raises(ValueError, match="siamese"):
        hf.cache_features(None, "siamese", [])


# ---------------------------------------------------------------------------------------------------------------------------------
# the operand refusals of `head_fit.step`, under the stub: nothing launches
# ---------------------------------------------------------------------------------------------------------------------------------
class _Cuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: all `_dev` / `_sized` ask of an operand before the library is reached."""
    @property
    def is_cuda(self):
        return True


def _gpu(t):
    return t.as_subclass(_Cuda)


@pytest.fixture
def stub(monkeypatch):
    """`operand_cases.install`'s stub behind `_lib.load`, and - this machine has no GPU - the two questions the wrapper asks the
    runtime answered without one: which device is current (`ops._on_operand_device`), and the current stream's handle."""
    monkeypatch.setattr(torch.cuda, "current_device", lambda: None)          # (a `_Cuda` tensor's device has index None)
    monkeypatch.setattr(hf, "_stream", lambda: 0)
    return oc.install(monkeypatch)


def _valid(amsgrad=False):
    N, B, D, C = 9, 4, 8, 3
    g = torch.Generator().manual_seed(1)
    return dict(x=torch.randn((N, D), generator=g), labels=torch.zeros((N,), dtype=torch.int32), w=torch.randn((C, D), generator=g),
                b=torch.zeros((C,)), state=torch.zeros((hf.state_bytes(D, C, amsgrad),), dtype=torch.uint8),
                workspace=torch.zeros((hf.workspace_bytes(B, D, C),), dtype=torch.uint8), rows=torch.tensor([0, 3, 8, 1], dtype=torch.int32),
                keep=torch.ones((B, D), dtype=torch.uint8))


DEPENDENT = {"labels": (0,), "w": (1,), "b": (0,), "state": (0,), "workspace": (0,), "keep": (0, 1)}


def _call(values, **kw):
    args = {k: (_gpu(v) if isinstance(v, torch.Tensor) and not isinstance(v, oc._OnCpu) else v) for k, v in values.items()}
    return hf.step(args["x"], args["labels"], args["w"], args["b"], args["state"], args["workspace"], args["rows"], args["keep"], 1.0 / 0.9,
                   lr=1e-3, **kw)


def test_the_valid_call_reaches_the_library(stub):
    with pytest.raises(oc.ReachedLibrary) as e:
        _call(_valid())
    assert e.value.entry == "frmap_head_fit_step" and e.value.args_[9:13] == (9, 4, 8, 3) and len(stub.calls) == 1
    with pytest.raises(oc.ReachedLibrary) as e:                       # without rows and keep: B is `batch`
        v = _valid()
        v["rows"] = v["keep"] = None
        _call(v, batch=4)
    assert e.value.args_[2] == 0 and e.value.args_[3] == 0 and e.value.args_[10] == 4


@pytest.mark.parametrize("operand", sorted(DEPENDENT))
def test_a_dependent_operand_is_refused_before_the_library(operand, stub):
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
    args = {k: _gpu(v) for k, v in values.items()}
    args[operand] = values[operand].clone()                           # this one stays a CPU tensor
    with pytest.raises(RuntimeError) as e:
        hf.step(args["x"], args["labels"], args["w"], args["b"], args["state"], args["workspace"], args["rows"], args["keep"], lr=1e-3)
    assert oc.names_operand(str(e.value), operand)
    assert stub.calls == []


def test_free_operands_and_batch_extent_are_refused(stub):
    for operand, bad, exc in (("x", torch.zeros((9,)), ValueError), ("x", torch.zeros((9, 8), dtype=torch.float64), TypeError),
                              ("rows", torch.zeros((2, 2), dtype=torch.int32), ValueError), ("rows", torch.zeros((4,), dtype=torch.int64), TypeError)):
        values = _valid()
        values[operand] = bad
        with pytest.raises(exc):
            _call(values)
    values = _valid()
    values["rows"] = values["keep"] = None
    with pytest.raises(ValueError, match="exceed"):
        _call(values, batch=10)
    # the AMSGrad state is larger: the plain one is refused with amsgrad=True
    with pytest.raises(ValueError, match="state"):
        _call(_valid(), amsgrad=True)
    with pytest.raises(ValueError):
        hf.LinearHead(0, 3, "cpu")
    with pytest.raises(ValueError):
        hf.LinearHead(8, hf.MAX_C + 1, "cpu")
    assert stub.calls == []


def test_linear_head_initialises_like_nn_linear():
    head = hf.LinearHead(512, 18, "cpu", generator=torch.Generator().manual_seed(7))
    bound = 1.0 / np.sqrt(512)
    assert head.weight.shape == (18, 512) and head.bias.shape == (18,) and head.weight.dtype == torch.float32
    assert float(head.weight.abs().max()) <= bound and float(head.bias.abs().max()) <= bound
    assert abs(float(head.weight.std()) - bound / np.sqrt(3)) < 0.05 * bound            # uniform in +-bound
    again = hf.LinearHead(512, 18, "cpu", generator=torch.Generator().manual_seed(7))
    assert torch.equal(head.weight, again.weight) and torch.equal(head.bias, again.bias)
    assert head.state.numel() == hf.state_bytes(512, 18) and not head.state.any() and sorted(head.state_dict()) == ["bias", "weight"]
    w, b = head.as_classifier()
    assert w is head.weight and b is head.bias
    fig = head.epoch_figures()
    assert fig["rows"] == 0 and fig["t"] == 0 and np.isnan(fig["accuracy"]) and np.isnan(fig["loss"])
    ref = torch.nn.Linear(512, 18)
    assert float(ref.weight.abs().max()) <= bound                                       # nn.Linear's own bound is the same
