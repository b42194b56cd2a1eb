"""GPU: every model walked layer by layer against its float64 rounding twin (`model_twin.py`), teacher-forced.

The walk IS production: the per-op plan's own forward (`face_models._PyTrunkPlan`, `_Py*Plan.embedding`) run with a recorder, which
is handed every stored tensor with the packed object or `ops` function that computed it; the labels are built here from those:

* recording changes nothing: the last recorded tensor is `torch.equal` to the module's own `get_embedding` (no recorder) on
  the per-op plan and on the default (handle) plan - on the hard weights too;
* every stored tensor within the bound the twin derives from the tensor the GPU stored for the step before: the one-rounding rule
  of `conv_cases.py` for conv / linear / stem / pool steps, the bars the fp32 heads, token and attention kernels already have
  for theirs (`model_twin.judge`); a `TWIN` line per step is printed before anything is asserted;
* end to end: the GPU's distance to the float64 oracle is at most twice the free-running twin's under its worst accumulation
  order (`model_twin.e2e_deviations`, computed on the CPU).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import frmap_amd  # noqa: E402
import frmap_amd.face_models as fm  # noqa: E402
from frmap_amd import _lib, ops, synth  # noqa: E402

import conv_cases as cc  # noqa: E402
import model_twin as mw  # noqa: E402

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
DT = {F16: "f16", BF16: "bf16"}
HARD = mw.HARD_VARIANTS[0]
# The batch of the large-batch row.  At 64 x 64 inputs (maps of 16 x 16 ... 2 x 2) the planner takes no second-generation
# (ping-pong) layout at B = 64: measured on an MI355X over B = 1 ... 2048, the first batch at which any layer of the trunk gets one
# is 298 (layer2's 3x3 convs on 8 x 8 x 128 maps, split-K layout 3).  The test asserts that one is taken.
PP_BATCH = 298


def _module(mt, sd, dtype, py_plan):
    m = frmap_amd.get_model(mt, 36)
    m.load_state_dict(sd)
    m = m.to(DEV).eval().set_compute_dtype(dtype)
    with fm.planned_in_python(py_plan):
        m._get_plan()
    return m


def _walk(mt, m, x):
    """`get_embedding` of the per-op module with a recorder: ([(name, stored tensor, kernel label)], the plan flags the twin mirrors)."""
    p, items = m._get_plan(), []
    assert p.handle is None and fm._HEAD_FUSE
    (p.pooled if mt == "cnn" else p.embedding)(m._check_input(x), lambda name, t, by, ins: items.append((name, t, _label(name, t, by, ins))))
    return items, mw.plan_flags([n for n, _, _ in items])


# ---- kernel labels from the planner's public queries, for what the recorder is handed ------------------------------------------
def _linear_label(M, K, N):
    return "linear_mfma split-K" if _lib.load().frmap_linear_mfma_workspace_bytes(M, K, N) > 0 else "linear_mfma"


def _stem_label(H, W):
    return "stem_s2d" if W % 4 == 0 and H >= 7 and W >= 7 else "stem_pool"


def _label(name, t, by, ins):
    """The label of step `name`, which stored `t`: `by` is the packed object (or `ops` function) that computed it from `ins`."""
    lib, x = _lib.load(), ins[0]
    if isinstance(by, fm._PackedLinearAsConv):
        return _linear_label(*x.shape, by.cout)
    if by is ops.conv_igemm:                                  # attention's q | k | v: a 1x1 conv on a bare packed weight
        return "conv1x1 pp=%d" % lib.frmap_conv1x1_pp_layout(*x.shape, t.shape[-1], 1)
    if isinstance(by, tuple):                                  # (conv2, downsample): the fused shortcut launch
        return "conv3x3_ds pp=%d" % lib.frmap_conv3x3_pp_ds_layout(*x.shape, by[0].cout, *ins[1].shape[1:], by[1].stride)
    if not isinstance(by, fm._PackedConv):
        return by.__name__                                     # an `ops` function
    if by.k == 7 and "+pool" in name:                          # the fused stems
        H, W = x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:]
        return _stem_label(H, W) + (" u8" if x.dtype == torch.uint8 else "")
    if name.endswith("+pool2"):
        return "small_cin_pool2" if by.small else "pool2 form=%d" % ops.conv_pool2_form(*x.shape, by.cout)
    if by.small:
        return f"small_cin k{by.k}"
    if by.k == 1:
        return "conv1x1 pp=%d" % lib.frmap_conv1x1_pp_layout(*x.shape, by.cout, by.stride)
    if by.stride == 2:
        return "conv3x3s2 pp=%d" % lib.frmap_conv3x3s2_pp_layout(*x.shape, by.cout)
    return "conv3x3 pp=%d" % lib.frmap_conv3x3_pp_layout(*x.shape, by.cout)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
# trunk families: the s2d stem (fp32 and bytes), the other fused stem (W % 4 != 0), the unfused stem (pooled width 58 > 56) with
# B = 1 maps on which the planner refuses the fused shortcut, and a batch at which second-generation layouts are planned
TRUNK_ROWS = [(3, 64, 64, False, (F16, BF16)), (3, 64, 64, True, (F16, BF16)), (3, 61, 37, False, (F16, BF16)),
              (1, 16, 232, False, (F16, BF16)), (PP_BATCH, 64, 64, False, (BF16,))]
CASES = [(mt, B, H, W, u8, dt) for mt in ("cnn", "arcface", "attention") for (B, H, W, u8, dts) in TRUNK_ROWS for dt in dts]
CASES += [("hybrid", 2, 224, 224, False, dt) for dt in (F16, BF16)]
CASES += [("baseline", 3, H, W, False, dt) for (H, W) in ((64, 64), (30, 22)) for dt in (F16, BF16)]     # 30 x 22: odd pooled sizes, conv and pool unfused
CASES += [("siamese", 2, n, n, False, dt) for n in (224, 15) for dt in (F16, BF16)]                      # 15: the smallest input the reference runs on
IDS = [f"{mt}-B{B}-{H}x{W}{'-u8' if u8 else ''}-{DT[dt]}" for (mt, B, H, W, u8, dt) in CASES]


def _inputs(mt, B, H, W, u8, dtype, m):
    """(what the module is given, the fp32 NCHW values the twin starts from)."""
    if u8:
        g = torch.Generator().manual_seed(8700 + H + W)
        img = torch.randint(0, 256, (B, H, W, 3), generator=g).to(torch.uint8).to(DEV)
        return img, ops.normalize_u8(img, m.input_mean, m.input_std)[0].to(dtype).float().cpu()
    x = synth.randn(8700 + len(mt) + H, (B, 3, H, W), "twin.gx")
    return x.to(DEV), x


@pytest.mark.parametrize("kind", ("cal", HARD))
@pytest.mark.parametrize("mt,B,H,W,u8,dtype", CASES, ids=IDS)
def test_walk_equals_production_and_every_step_meets_its_bound(mt, B, H, W, u8, dtype, kind, calibrated_sd):
    sd = mw.weights_of(kind, mt, calibrated_sd(mt))
    m_py, m_h = _module(mt, sd, dtype, True), _module(mt, sd, dtype, False)
    x_dev, x_twin = _inputs(mt, B, H, W, u8, dtype, m_py)
    with torch.no_grad():
        items, plan = _walk(mt, m_py, x_dev)
        cc._sync(f"{mt} walk")
        last = items[-2 if mt == "baseline" else -1][1]
        for what, m in (("per-op plan", m_py), ("handle plan", m_h)):
            e = m.get_embedding(x_dev)
            assert torch.equal(e.reshape(last.shape), last), (what, "get_embedding differs from the recorded run")
        if mt == "baseline":
            assert torch.equal(m_py.unit_embedding(x_dev), items[-1][1])    # (the handle normalises its embedding in a launch of its own)
        cc._sync(f"{mt} get_embedding")
    if mt != "attention":
        assert m_h.model_handle() is not None and m_py.model_handle() is None
    forced = [mw.to_twin_layout(t) for _, t, _ in items]
    steps = mw.run(mt, sd, x_twin, dtype, plan, forced=forced)
    assert [s.name for s in steps] == [n for n, _, _ in items]
    failures, labels = [], []
    for s, y, (_, _, label) in zip(steps, forced, items):
        frac, err = (mw.ratio(s, y, dtype) if s.kind == "round" else float("nan")), None
        try:
            frac = mw.judge(s, y, dtype, s.name)
        except AssertionError as e:
            err = e
        print(f"TWIN {mt} {DT[dtype]} {kind} {B}x{H}x{W}{'u8' if u8 else ''} {s.name} [{label}] {frac:.3f}" + (" FAILS" if err is not None else ""))
        labels.append(label)
        if err is not None:
            failures.append((s.name, label, str(err)[:300]))
    assert not failures, failures
    if (B, H, W) == (1, 16, 232):
        assert not plan["stem_fused"] and not all(plan["ds_fused"]), plan          # the row's reason: unfused stem, an unfused shortcut
    if B == PP_BATCH:
        assert any(" pp=" in lb and not lb.endswith("pp=0") for lb in labels), ("no second-generation layout at this batch", labels)
    if mt == "baseline":
        assert plan["pool_fused"] == ((True, True, True) if (H, W) == (64, 64) else (True, False, False)), plan


@pytest.mark.parametrize("kind", ("cal", HARD))
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("mt", mw.MODELS)
def test_end_to_end_deviation_is_within_twice_the_twins(mt, dtype, kind, calibrated_sd):
    """E_hip = rel-L2(GPU embedding, float64 oracle) <= 2 max_v E_v, E_v the free-running twin's under float64, sequential,
    chunked and reversed fp32 accumulation (the factor 2: the power-of-two headroom C_ACC has over its CPU restatements)."""
    sd = mw.weights_of(kind, mt, calibrated_sd(mt))
    x = mw.e2e_input(mt)
    m, m_py = _module(mt, sd, dtype, False), _module(mt, sd, dtype, True)
    with torch.no_grad():
        emb = m.get_embedding(x.to(DEV)).float().cpu().reshape(x.shape[0], -1)
        plan = _walk(mt, m_py, x.to(DEV))[1]                             # which launches the planner fuses at this shape
    cc._sync(f"{mt} end to end")
    oracle = mw.oracle64(mt, sd, x)
    E = mw.e2e_deviations(mt, sd, x, dtype, plan, oracle)
    e_hip = mw.rel_l2(emb, oracle)
    print(f"TWINE2E {mt} {DT[dtype]} {kind} B={x.shape[0]} " + " ".join(f"{v}={E[v]:.3e}" for v in mw.ACC_VARIANTS) + f" E_hip={e_hip:.3e} "
          f"E_hip/max={e_hip / max(E.values()):.3f}")
    assert e_hip <= 2.0 * max(E.values()), (e_hip, E)
