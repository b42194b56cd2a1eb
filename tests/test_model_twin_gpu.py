"""GPU: every model walked layer by layer against its float64 rounding twin (`model_twin.py`), teacher-forced.

The walk runs the per-op plan's own packed objects (`_PyTrunkPlan.stem` / `.blocks`, the dict plans of BaselineNet, SiameseNet,
HybridNet, AttentionNet) through the calls `forward` / `get_embedding` make, in their order, and keeps every intermediate:

* same walk as production: its last tensor is `torch.equal` to the module's own `get_embedding` on the per-op plan and on the
  default (handle) plan - on the hard weights too;
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
    old = fm._PY_PLAN
    fm._PY_PLAN = bool(py_plan)
    try:
        m._get_plan()
    finally:
        fm._PY_PLAN = old
    return m


class Rec:
    """The stored tensors of one walk: (name, tensor, kernel label)."""

    def __init__(self):
        self.items = []

    def __call__(self, name, t, label):
        self.items.append((name, t, label))
        return t


# ---- kernel labels from the planner's public queries ---------------------------------------------------------------------------
def _label(conv, x, ds_x=None, ds=None):
    lib = _lib.load()
    B, H, W, C = x.shape
    if conv.small:
        return f"small_cin k{conv.k}"
    if ds is not None:
        return "conv3x3_ds pp=%d" % lib.frmap_conv3x3_pp_ds_layout(B, H, W, C, conv.cout, ds_x.shape[1], ds_x.shape[2], ds_x.shape[3], ds.stride)
    if conv.k == 1:
        return "conv1x1 pp=%d" % lib.frmap_conv1x1_pp_layout(B, H, W, C, conv.cout, conv.stride)
    if conv.stride == 2:
        return "conv3x3s2 pp=%d" % lib.frmap_conv3x3s2_pp_layout(B, H, W, C, conv.cout)
    return "conv3x3 pp=%d" % lib.frmap_conv3x3_pp_layout(B, H, W, C, conv.cout)


def _linear_label(M, K, N):
    return "linear_mfma split-K" if _lib.load().frmap_linear_mfma_workspace_bytes(M, K, N) > 0 else "linear_mfma"


def _stem_label(H, W):
    return "stem_s2d" if W % 4 == 0 and H >= 7 and W >= 7 else "stem_pool"


# ---- the walks -----------------------------------------------------------------------------------------------------------------
def _walk_trunk(tp, x, rec, plan):
    u8 = x.dtype == torch.uint8
    H, W = (x.shape[1], x.shape[2]) if u8 else (x.shape[2], x.shape[3])
    plan["stem_fused"] = ops.stem_pool_dims(H, W)[1] <= 56 and (not u8 or W % 4 == 0)
    if plan["stem_fused"] and u8:
        x = rec("stem+pool3", ops.stem7x7_maxpool_u8(x, tp.stem.wpk, tp.stem.shift, tp.mean, tp.std, tp.dtype), _stem_label(H, W) + " u8")
    elif plan["stem_fused"]:
        x = rec("stem+pool3", ops.stem7x7_maxpool(x, tp.stem.wpk, tp.stem.shift, tp.dtype), _stem_label(H, W))
    else:
        assert not u8
        x4 = rec("pack_input", ops.pack_input(x, tp.dtype), "pack_input")
        c = rec("stem", tp.stem(x4, relu=True), _label(tp.stem, x4))
        x = rec("stem.pool3", ops.maxpool(c, 3, 2, 1), "maxpool")
    fused = []
    for i, (c1, c2, ds, fshift) in enumerate(tp.blocks):
        name = f"layer{i // 2 + 1}.{i % 2}."
        if ds is None:
            a = rec(name + "conv1", c1(x, relu=True), _label(c1, x))
            x = rec(name + "conv2", c2(a, relu=True, residual=x), _label(c2, a))
            continue
        h = rec(name + "conv1", c1(x, relu=True), _label(c1, x))
        B, Hh, Wh, Ch = h.shape
        fused.append(ds.k == 1 and ops.conv_ds_supported(B, Hh, Wh, Ch, c2.cout, x.shape[1], x.shape[2], x.shape[3], ds.stride))
        if fused[-1]:
            x = rec(name + "conv2+ds", ops.conv_igemm_ds(h, c2.wpk, fshift, c2.cout, x, ds.wpk, ds.stride, True), _label(c2, h, x, ds))
        else:
            d = rec(name + "downsample", ds(x, relu=False), _label(ds, x))
            x = rec(name + "conv2", c2(h, relu=True, residual=d), _label(c2, h))
    plan["ds_fused"] = tuple(fused)
    return x


def _walk_pooled(rec, name, conv, x, fused_list):
    B, H, W, C = x.shape
    fusable = conv.k == 3 and conv.stride == 1 and conv.pad == 1 and H % 2 == 0 and W % 2 == 0 and fm._POOL_FUSE
    if fusable and conv.small and conv.cout == 32:
        fused_list.append(True)
        return rec(name + "+pool2", ops.conv_small_cin_pool2(x, conv.wpk, conv.shift, conv.cout, True), "small_cin_pool2")
    if fusable and not conv.small and ops.conv_pool2_supported(B, H, W, C, conv.cout):
        fused_list.append(True)
        return rec(name + "+pool2", ops.conv_igemm_pool2(x, conv.wpk, conv.shift, conv.cout, True), "pool2 form=%d" % ops.conv_pool2_form(B, H, W, C, conv.cout))
    fused_list.append(False)
    c = rec(name, conv(x, relu=True), _label(conv, x))
    return rec(name + ".pool2", ops.maxpool(c, 2, 2, 0), "maxpool")


def _walk(mt, m, x, rec):
    """The calls of `get_embedding` on the per-op plan, every intermediate recorded.  Returns the plan flags the twin mirrors."""
    p = m._get_plan()
    plan = {}
    x = m._check_input(x)
    if mt == "cnn":
        assert isinstance(p, fm._PyTrunkPlan)
        rec("avgpool", ops.avgpool_global(_walk_trunk(p, x, rec, plan)), "avgpool_global")
    elif mt == "arcface":
        f = _walk_trunk(p["trunk"], x, rec, plan)
        assert fm._HEAD_FUSE and p["wt"].shape[1] == 512
        rec("embedding+bn+normalize", ops.gap_linear_norm(f, p["wt"], p["bn_scale"], p["bn_shift"], 1e-12)[0], "gap_linear_norm")
    elif mt == "attention":
        f = _walk_trunk(p["trunk"], x, rec, plan)
        qkv = rec("attention.qkv", ops.conv_igemm(f, p["qkv"], p["qkv_bias"], p["cqkv"], 1, 1, 0, 0),
                  "conv1x1 pp=%d" % _lib.load().frmap_conv1x1_pp_layout(*f.shape, p["cqkv"], 1))
        rec("attention.pool", ops.cnn_attention(qkv, f, p["gamma"], p["sw"], p["sb"], p["cq"], want_map=False, want_pool=True)[1], "cnn_attention")
    elif mt == "hybrid":
        f = _walk_trunk(p["trunk"], x, rec, plan)
        B, Hh, Ww, D = f.shape
        L = Hh * Ww
        assert L == m.seq_len
        t, n1 = ops.add_pos_layernorm(f.view(B, L, D), p["pos"], *p["n1"], want_sum=True)
        rec("tokens+pos", t, "add_pos_layernorm")
        rec("norm1", n1, "add_pos_layernorm")
        qkv = rec("in_proj", p["qkv"](n1.view(B * L, D), relu=0), _linear_label(B * L, D, 3 * D))
        att = rec("mha", ops.mha_tokens(qkv.view(B, L, 3 * D), m.transformer.attention.num_heads), "mha_tokens")
        t2 = rec("out_proj+res", p["proj"](att.view(B * L, D), relu=0, residual=t.view(B * L, D)), _linear_label(B * L, D, D))
        n2 = rec("norm2", ops.add_pos_layernorm(t2.view(B, L, D), None, *p["n2"])[1], "add_pos_layernorm")
        hdn = rec("ff.0+gelu", p["ff1"](n2.view(B * L, D), relu=2), _linear_label(B * L, D, 2048))
        t3 = rec("ff.3+res", p["ff2"](hdn, relu=0, residual=t2), _linear_label(B * L, 2048, D))
        rec("mean+norm", ops.mean_layernorm(t3.view(B, L, D), *p["nf"]), "mean_layernorm")
    elif mt == "baseline":
        assert isinstance(p, dict) and fm._HEAD_FUSE
        h = rec("pack_input", m._as_nhwc4(x), "pack_input")
        fused = []
        for i in (1, 2, 3):
            h = _walk_pooled(rec, f"conv{i}", p[f"c{i}"], h, fused)
        plan["pool_fused"] = tuple(fused)
        emb, pre = ops.gap_linear_norm(h, p["fc1_t"], None, m.fc1.bias.detach(), 1e-12, want_pre=True, relu=True)
        rec("fc1+relu", pre, "gap_linear_norm")
        rec("fc1+relu.unit", emb, "gap_linear_norm")
    elif mt == "siamese":
        convs = p["convs"]
        Wi = x.shape[3]
        plan["stem_fused"] = ((Wi + 6 - 7) // 2 + 1) // 2 <= 64
        fused = []
        if plan["stem_fused"]:
            h = rec("conv.0+pool2", ops.stem7x7_maxpool(x, convs[0][0].wpk, convs[0][0].shift, m.compute_dtype, pool3=False), _stem_label(x.shape[2], Wi))
        else:
            h = _walk_pooled(rec, "conv.0", convs[0][0], rec("pack_input", m._as_nhwc4(x), "pack_input"), [])
        for (conv, pool), (ci, _, _) in zip(convs[1:], mw.SIAMESE_CONVS):
            h = _walk_pooled(rec, f"conv.{ci}", conv, h, fused) if pool else rec(f"conv.{ci}", conv(h, relu=True), _label(conv, h))
        plan["pool_fused"] = tuple(fused)
        a = rec("avgpool6x6", ops.avgpool_adaptive(h, 6, 6), "avgpool_adaptive")
        B = a.shape[0]
        f = rec("fc.1", p["fc1"](a.view(B, -1), relu=True), _linear_label(B, 18432, 1024))
        f = rec("fc.5", p["fc2"](f, relu=True), _linear_label(B, 1024, 512))
        f = rec("fc.8", p["fc3"](f, relu=False), _linear_label(B, 512, 256))
        f = rec("cast_f32", ops.cast_to_f32(f), "cast_to_f32")
        rec("normalize", ops.l2_normalize(f, 1e-12), "l2_normalize")
    else:
        raise ValueError(mt)
    return plan


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
    rec = Rec()
    with torch.no_grad():
        plan = _walk(mt, m_py, x_dev, rec)
        cc._sync(f"{mt} walk")
        last = rec.items[-2 if mt == "baseline" else -1][1]
        for what, m in (("per-op plan", m_py), ("handle plan", m_h)):
            e = m.get_embedding(x_dev)
            assert torch.equal(e.reshape(last.shape), last), (what, "get_embedding differs from the walk")
        if mt == "baseline":
            assert torch.equal(m_py.unit_embedding(x_dev), rec.items[-1][1])    # (the handle normalises its embedding in a launch of its own)
        cc._sync(f"{mt} get_embedding")
    if mt != "attention":
        assert m_h.model_handle() is not None and m_py.model_handle() is None
    forced = [mw.to_twin_layout(t) for _, t, _ in rec.items]
    steps = mw.run(mt, sd, x_twin, dtype, plan, forced=forced)
    assert [s.name for s in steps] == [n for n, _, _ in rec.items]
    failures, labels = [], []
    for s, y, (_, _, label) in zip(steps, forced, rec.items):
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
        plan = _walk(mt, m_py, x.to(DEV), Rec())                         # which launches the planner fuses at this shape
    cc._sync(f"{mt} end to end")
    oracle = mw.oracle64(mt, sd, x)
    E = mw.e2e_deviations(mt, sd, x, dtype, plan, oracle)
    e_hip = mw.rel_l2(emb, oracle)
    print(f"TWINE2E {mt} {DT[dtype]} {kind} B={x.shape[0]} " + " ".join(f"{v}={E[v]:.3e}" for v in mw.ACC_VARIANTS) + f" E_hip={e_hip:.3e} "
          f"E_hip/max={e_hip / max(E.values()):.3f}")
    assert e_hip <= 2.0 * max(E.values()), (e_hip, E)
