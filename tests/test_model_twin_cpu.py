"""CPU: the float64 rounding twin of the six models (`model_twin.py`) on its own - no kernel runs here.

* the hard weights are hard and legal: every class in every BatchNorm with >= 2 channels, opposed shortcut shifts, >= 1000
  subnormal fp16 weights per model, every stored tensor finite and below the dtype's maximum, zero-gamma channels constant,
  more than 10 % of every post-ReLU tensor alive;
* the acceptance rules reject wrong assemblies: eleven mutated twins, each compared teacher-forced with the correct twin's stored
  tensors, miss their first affected step by >= 2 x the bound on the hard weights (`TWINMUT` lines; the ratio on the calibrated
  weights is printed beside it, not asserted: DESIGN.md section 2 lists which mutants those let through);
* the end-to-end allowance: the free-running twin's distance to the float64 oracle under four accumulation orders (`TWINE2E`
  lines), which must agree within 2 x among themselves;
* the handle path refuses a BatchNorm whose eps is not the 1e-5 `frmap_model_finalize` folds with.
"""
import pytest
import torch

import frmap_amd
import frmap_amd.face_models as fm
from oracle import face_oracle as fo

import conv_cases as cc
import model_twin as mw

DTYPES = [torch.float16, torch.bfloat16]
DT = {torch.float16: "f16", torch.bfloat16: "bf16"}
# the smallest input at which each model runs every branch of its assembly (hybrid needs 49 tokens: 224 x 224)
SHAPE = {"baseline": (2, 30, 22), "cnn": (2, 64, 64), "arcface": (2, 64, 64), "attention": (2, 64, 64), "siamese": (2, 15, 15),
         "hybrid": (1, 224, 224)}
SIAMESE_MIN = 15


def _x(mt, shape=None, seed=8800):
    B, H, W = shape or SHAPE[mt]
    return frmap_amd.synth.randn(seed + len(mt), (B, 3, H, W), "twin.x")


_runs = {}


def _free(mt, kind, dtype, calibrated_sd):
    """The correct twin, free-running, once per (model, weights, dtype): (weights, steps)."""
    key = (mt, kind, dtype)
    if key not in _runs:
        sd = mw.weights_of(kind, mt, calibrated_sd(mt))
        _runs[key] = (sd, mw.run(mt, sd, _x(mt), dtype))
    return _runs[key]


# ------------------------------------------------------------------------------------------------------------------------------
# hard weights
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", mw.HARD_VARIANTS)
@pytest.mark.parametrize("mt", mw.MODELS)
def test_hard_weights_hold_every_class_in_every_layer(mt, variant, calibrated_sd):
    cal = calibrated_sd(mt)
    sd = mw.hard_state_dict(mt, cal, variant)
    assert set(sd) == set(cal) and all(sd[k].shape == cal[k].shape for k in sd)
    chans = mw.hard_channels(cal, variant)
    assert sorted(chans) == sorted(mw.bn_prefixes(cal)) and chans
    n_sub = 0
    for p, cls in chans.items():
        g, var, mean = sd[p + "weight"], sd[p + "running_var"], sd[p + "running_mean"]
        want = [c for c in mw.CLASSES if c != "bias" or mw.bias_key_of(cal, p) is not None]
        used = [c for n in want for c in cls[n]]
        assert all(len(cls[n]) >= 2 for n in want) and len(set(used)) == len(used), (p, cls)
        assert bool(((var[cls["tiny_var"]] >= 1e-6) & (var[cls["tiny_var"]] <= 1e-4)).all()), p
        assert bool((g[cls["neg_gamma"]] < 0).all()) and bool((g[cls["zero_gamma"]] == 0).all()), p
        scale, shift = mw.bn_fold(sd, p)
        ms = (mean * scale).abs()[cls["big_mean"]]
        out_sigma = (scale.abs() * torch.sqrt(var))[cls["big_mean"]]
        assert bool((ms > 20 * out_sigma).all()) and bool((g[cls["big_mean"]].abs() < 0.1).all()), (p, ms)     # mean * scale is > 20 sigma of the output
        assert bool(((g[cls["small_gamma"]].abs() > 5e-5) & (g[cls["small_gamma"]].abs() < 2e-4)).all()), p
        assert bool(torch.isfinite(scale).all()) and bool(torch.isfinite(shift).all()), p
        bk = mw.bias_key_of(cal, p)
        if bk is not None:
            b = sd[bk][cls["bias"]]
            assert bool((b != 0).all()) and bool(((b * scale[cls["bias"]] - b).abs() > 1.0 * torch.sqrt(var[cls["bias"]])).all()), p
        if "shortcut" in cls and p.endswith("bn2."):
            d = p[:-len("bn2.")] + "downsample.1."
            s2, sds = shift[cls["shortcut"]], mw.bn_fold(sd, d)[1][cls["shortcut"]]
            assert len(cls["shortcut"]) >= 2 and bool((s2 * sds < 0).all()), (p, s2, sds)                # differ in sign ...
            r = s2.abs() / sds.abs()
            assert bool(((r > 2) | (r < 0.5)).all()), (p, r)                                             # ... and in size
    for k in (k for k in cal if k.endswith(".bias") and "norm" not in k):
        if not any(k == p + "bias" for p in chans):
            assert int((sd[k] != 0).sum()) >= min(2, sd[k].numel()), k
    if mt in mw.TRUNK_PREFIX:
        blocks = [p for p, cls in chans.items() if "shortcut" in cls and p.endswith("bn2.")]
        assert sorted(p.split(".")[-4] for p in blocks) == ["layer2", "layer3", "layer4"], blocks
    for k in cal:                                            # subnormal, non-zero fp16 folded weights (the fold of the twin)
        bnp = _bn_of_weight(cal, k)
        if bnp is not None:
            w = (sd[k].float() * mw.bn_fold(sd, bnp)[0].view(-1, *([1] * (sd[k].dim() - 1)))).to(torch.float16).float().abs()
            n_sub += int(((w > 0) & (w < 2.0 ** -14)).sum())
    print(f"TWINHARD {mt} {variant}: {len(chans)} BatchNorms, {n_sub} subnormal non-zero folded fp16 weights")
    assert n_sub >= 1000


def _bn_of_weight(sd, k):
    """The BatchNorm that folds into conv / linear weight `k` (the inverse of `bias_key_of`, by name), or None."""
    if not k.endswith(".weight") or sd[k].dim() < 2 or k.startswith("features."):
        return None
    parts = k[:-len(".weight")].split(".")
    if parts[-1].isdigit():
        cand = ".".join(parts[:-1] + [str(int(parts[-1]) + 1)]) + "."
    elif parts[-1].startswith("conv") and parts[-1][4:].isdigit():
        cand = ".".join(parts[:-1] + ["bn" + parts[-1][4:]]) + "."
    else:
        return None
    return cand if (cand + "running_var") in sd and sd[cand + "running_var"].shape[0] == sd[k].shape[0] else None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", mw.HARD_VARIANTS)
@pytest.mark.parametrize("mt", mw.MODELS)
def test_hard_twin_is_finite_alive_and_constant_where_gamma_is_zero(mt, variant, dtype, calibrated_sd):
    sd, steps = _free(mt, variant, dtype, calibrated_sd)
    chans = mw.hard_channels(calibrated_sd(mt), variant)
    top = torch.finfo(dtype).max
    for st in steps:
        assert bool(torch.isfinite(st.value).all()) and float(st.value.abs().max()) < top, (st.name, float(st.value.abs().max()))
        if st.kind == "round":
            assert bool(torch.isfinite(st.want).all()) and float(cc.act64(st.want, st.act).abs().max()) < top, st.name
            if st.act == cc.ACT_RELU or "pool" in st.name:
                alive = float((st.value != 0).double().mean())
                assert alive > 0.10, (st.name, alive)
        bn = st.meta.get("bn")
        if bn is not None:                                   # a BatchNorm-folded step without a residual: gamma = 0 leaves act(shift)
            bk = mw.bias_key_of(sd, bn)
            shift = mw.bn_fold(sd, bn, sd[bk] if bk is not None else None)[1]
            for c in chans[bn]["zero_gamma"]:
                v = st.value[:, c]
                want = float(shift[c]) if st.name.endswith("downsample") else max(float(shift[c]), 0.0)
                assert float(v.max()) == float(v.min()) == float(torch.tensor(want).to(dtype)), (st.name, c, float(v.max()), want)


def test_siamese_smallest_input_is_15():
    """The smallest square input the reference's SiameseNet runs on: three 2 x 2 pools behind a stride-2 conv need 8 conv rows."""
    sd = {k: torch.zeros(s, dtype=d) for k, (s, d) in frmap_amd.synth.shapes_of(frmap_amd.get_model("siamese")).items()}
    for k in sd:
        if k.endswith("running_var"):
            sd[k] += 1.0

    def runs(n):
        try:
            with torch.no_grad():
                fo.siamese_forward_one(sd, torch.zeros(1, 3, n, n))
            return True
        except RuntimeError:
            return False
    assert [n for n in range(1, 20) if runs(n)][0] == SIAMESE_MIN == SHAPE["siamese"][1]


# ------------------------------------------------------------------------------------------------------------------------------
# the rule rejects wrong assemblies
# ------------------------------------------------------------------------------------------------------------------------------
MUTANTS = [("no_eps", "cnn"), ("eps_1e-3", "cnn"), ("bias_unscaled", "baseline"), ("bias_unscaled", "siamese"), ("drop_mean", "cnn"),
           ("no_ds_shift_2", "cnn"), ("no_ds_shift_3", "cnn"), ("no_ds_shift_4", "cnn"), ("res_conv1", "cnn"), ("res_after_round", "cnn"),
           ("slot", "cnn"), ("no_perm", "siamese"), ("pool_swap", "cnn"), ("qkv_order", "attention")]


def _first_affected(mt, kind, dtype, mutant, calibrated_sd):
    """(step name, ratio) at the first step whose reference the mutation changes, both twins fed the correct twin's stored tensors."""
    sd, good = _free(mt, kind, dtype, calibrated_sd)
    stored = [s.value for s in good]
    bad = mw.run(mt, sd, _x(mt), dtype, mut=(mutant,), forced=stored)
    assert [s.name for s in bad] == [s.name for s in good]
    for g, b, y in zip(good, bad, stored):
        if g.kind != "round":
            continue
        if not (torch.equal(g.want, b.want) and torch.equal(g.S, b.S)):
            return g, b, y
    raise AssertionError(f"{mutant} changes no step of {mt}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant,mt", MUTANTS)
def test_mutated_assembly_misses_its_first_affected_step_by_2x(mutant, mt, dtype, calibrated_sd):
    for kind in ("cal", mw.HARD_VARIANTS[0]):
        g, b, y = _first_affected(mt, kind, dtype, mutant, calibrated_sd)
        assert mw.judge(g, y, dtype, g.name) <= 1.0                      # the correct twin passes the rule it is held to (slack check included)
        r = mw.ratio(b, y, dtype)
        print(f"TWINMUT {mutant} {mt} {DT[dtype]} {g.name} {r:.3g} ({'calibrated, not asserted' if kind == 'cal' else 'hard'})")
        # what an end-to-end gate sees of the same mutant: its free-running embedding's distance to the float64 oracle, in units of the
        # correct twin's (2.5 = the regression gate of test_models_gpu.py); printed, not asserted
        sd, good = _free(mt, kind, dtype, calibrated_sd)
        oracle = mw.oracle64(mt, sd, _x(mt))
        e_good = mw.rel_l2(mw.embedding_of(mt, good), oracle)
        e_bad = mw.rel_l2(mw.embedding_of(mt, mw.run(mt, sd, _x(mt), dtype, mut=(mutant,))), oracle)
        print(f"TWINMUT-E2E {mutant} {mt} {DT[dtype]} {kind} E_mutant/E_twin = {e_bad / e_good:.3g}")
        if kind != "cal":
            assert r >= 2.0, (mutant, mt, g.name, r)
            with pytest.raises(AssertionError, match="reaches"):
                mw.judge(b, y, dtype, f"{mutant} {g.name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ("cal",) + mw.HARD_VARIANTS[:1])
@pytest.mark.parametrize("mt", mw.MODELS)
def test_correct_twin_meets_every_rule_it_states(mt, kind, dtype, calibrated_sd):
    """Every step of the free-running twin passes its own acceptance rule (for the one-rounding rule that includes the check that
    the case keeps the rule sharp), and a teacher-forced run on its own tensors reproduces them."""
    sd, steps = _free(mt, kind, dtype, calibrated_sd)
    again = mw.run(mt, sd, _x(mt), dtype, forced=[s.value for s in steps])
    for s, a in zip(steps, again):
        assert torch.equal(s.value, a.value), s.name
        assert mw.judge(s, s.value, dtype, f"{mt} {kind} {s.name}") <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# the end-to-end allowance
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ("cal",) + mw.HARD_VARIANTS[:1])
@pytest.mark.parametrize("mt", mw.MODELS)
def test_accumulation_order_moves_the_twin_by_less_than_2x(mt, kind, dtype, calibrated_sd):
    """E_v = rel-L2(twin embedding, float64 oracle) under float64, sequential fp32, chunked fp32 and reversed fp32 accumulation.
    The GPU gate is E_hip <= 2 max_v E_v; a spread above 2 x among the E_v would mean the batch is too small for the statistic."""
    sd = mw.weights_of(kind, mt, calibrated_sd(mt))
    E = mw.e2e_deviations(mt, sd, mw.e2e_input(mt), dtype)
    spread = max(E.values()) / min(E.values())
    print(f"TWINE2E {mt} {DT[dtype]} {kind} B={mw.E2E_SHAPE[mt][0]} " + " ".join(f"{v}={E[v]:.3e}" for v in mw.ACC_VARIANTS) + f" spread={spread:.3f}")
    assert min(E.values()) > 0 and spread <= 2.0, (E, spread)


# ------------------------------------------------------------------------------------------------------------------------------
# the handle folds with eps = 1e-5: a module that says otherwise is refused
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt,layer", [("cnn", "resnet.layer2.0.downsample.1"), ("arcface", "bn"), ("baseline", "bn2"), ("siamese", "fc.6"),
                                      ("hybrid", "cnn.layer4.1.bn2"), ("attention", "backbone.layer1.0.bn1")])
def test_handle_plan_refuses_a_batchnorm_with_another_eps(mt, layer):
    m = frmap_amd.get_model(mt, 36).eval()
    m.get_submodule(layer).eps = 1e-3
    with fm.planned_in_python(False), pytest.raises(ValueError, match=layer.replace(".", r"\.") + r".*eps"):
        m._build_plan(torch.float16)


# ------------------------------------------------------------------------------------------------------------------------------
# the plan flags the GPU test hands the twin are read off step names
# ------------------------------------------------------------------------------------------------------------------------------
def _plans(mt):
    """Every plan the HIP path can take for the family (only the flags it has steps for)."""
    ds = [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)]
    if mt == "baseline":
        return [{"pool_fused": pf} for pf in ds]
    if mt == "siamese":
        return [{"stem_fused": s, "pool_fused": pf} for s in (True, False) for pf in sorted({d[:2] for d in ds})]
    if mt == "hybrid":          # (needs its 49 tokens, a 224 x 224 input: the plan of its GPU cases)
        return [{"stem_fused": True, "ds_fused": ds[0]}]
    return [{"stem_fused": s, "ds_fused": d} for s in (True, False) for d in (ds if mt == "cnn" else ds[:1] + ds[-1:])]


@pytest.mark.parametrize("mt", mw.MODELS)
def test_plan_flags_are_read_off_the_step_names(mt):
    """`mw.plan_flags` on the names the twin records under a plan gives that plan back, for every plan the GPU test's cases can
    meet (the names depend on the plan alone, so a small input serves)."""
    sd = frmap_amd.synth.synth_state_dict(frmap_amd.synth.shapes_of(frmap_amd.get_model(mt, 36)), 8900)
    x = _x(mt, None if mt == "hybrid" else (1, 32, 32))
    for plan in _plans(mt):
        names = [s.name for s in mw.run(mt, sd, x, torch.float16, plan)]
        assert mw.plan_flags(names) == {"stem_fused": False, "ds_fused": (), "pool_fused": (), **plan}, (plan, names)


def test_header_states_the_eps_the_handle_folds_with():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frmap_hip.h")).read()
    doc = text[text.index("frmap_model_finalize     folds"):text.index("frmap_model_forward      x:")]
    assert "eps = 1e-5" in doc and "state_dict does not carry eps" in doc
    assert fm.HANDLE_BN_EPS == mw.BN_EPS == 1e-5
