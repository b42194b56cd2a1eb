"""GPU: what every wrapper of `ops` does with the tensors it is handed (`operand_cases.py`).

The binding turns a `torch.Tensor` into a bare pointer and hands it to the library with integers that describe ANOTHER tensor; the
library cannot see how long a `shift`, `gamma`, `pos`, `scale` or `w` really is.  Four parts.

1. Strided operands give the bits of the contiguous call.  Every two-fill test of `test_guard_ops_gpu.py` and `test_guard_conv_gpu.py`
   (all of their cases) runs again under `place_cases.strided_rule`: every placed operand at once a `wide[..., ::2]` view - the binding
   copies each, and all the copies of one call are alive together - and, where the case has 4-D operands, once more with those as the
   `permute(0, 2, 3, 1)` view of a tensor laid out the other way round.  Bit identity with the call on clones
   (`guard.first_difference`); no tolerance.  Stride-0 `expand`s of per-channel vectors and of `pos` have a test of their own.
2. A tensor the call WRITES is refused in aligned, non-contiguous form and never copied: ValueError, the caller's buffer untouched,
   the library not reached (`StubLibrary`); then the same call on the contiguous tensor, through the real library, updates that
   tensor where it is.
3. A bad DEPENDENT operand - too short by one, too long by one, wrong rank, wrong dtype, on the CPU - is refused before the library
   with the exception `_dev`'s convention sets and a message that names it, for every (wrapper, dependent operand) of the table; the
   valid call reaches the library, so the refusal was that operand's.  All under `StubLibrary`: nothing is launched, a wrapper that
   fails to refuse is reported and not run out of bounds.  The test ids carry k / n of the table's (wrapper, dependent operand) pairs.
4. Device: on a host with two GPUs every row's call with its operands on `cuda:1` while `cuda:0` is current - positional, keyword
   and prepared-gallery operands - returns the bits of the call made with `cuda:1` current.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
import guard  # noqa: E402
import operand_cases as oc  # noqa: E402
import place_cases as pc  # noqa: E402
import test_guard_conv_gpu as tgc  # noqa: E402
import test_guard_ops_gpu as tgo  # noqa: E402
from frmap_amd import ops, synth  # noqa: E402

DEV = "cuda"


def _to(device):
    return lambda t: t.to(device, copy=True)


def _same_bits(got, ref, what):
    got, ref = guard._flat(got), guard._flat(ref)
    assert len(got) == len(ref), (what, len(got), len(ref))
    for k in range(len(ref)):
        d = guard.first_difference(got[k], ref[k])
        assert d is None, "%s: result %d: %s" % (what, k, d)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. strided operands
# ---------------------------------------------------------------------------------------------------------------------------------
OPS_TESTS = [n for n in dir(tgo) if n.startswith("test_") and n != "test_positive_control_one_element_too_many"]
CONV_TESTS = [n for n in dir(tgc) if n.startswith("test_") and n != "test_linear_case_is_guarded"]
assert len(OPS_TESTS) >= 20 and len(CONV_TESTS) == 4

for _name in OPS_TESTS:
    globals()[_name + "_on_strided_views"] = pc.mirror_strided(tgo, _name)
for _name in CONV_TESTS:
    globals()[_name.replace("_is_guarded", "_on_strided_views")] = pc.mirror_strided(tgc, _name)
del _name


@pytest.mark.parametrize("dtype", tgc.DTYPES, ids=tgc.DT_IDS)
@pytest.mark.parametrize("lc", cc.LINEAR_CASES, ids=[c.name for c in cc.LINEAR_CASES])
def test_linear_case_on_strided_views(lc, dtype):
    """(the guard test also counts the guard's allocations, which views do not have: `cc.run_linear` under the rule itself)"""
    o = cc.linear_operands(lc, "gauss" if lc.act == cc.ACT_GELU else "exact", dtype)
    pc.strided_rule(lambda place: cc.run_linear(lc, o, dtype, place=place), what=lc.name)


def test_stride_zero_vectors_give_the_bits_of_the_contiguous_call():
    """Per-channel vectors of one repeated value as the `expand` of a one-element source, `pos` of one repeated row as the `expand`
    of a one-row source: three stride-0 operands of equal size in one call."""
    B, L, D, N = 2, 5, 64, 64
    ex, dev = lambda t: oc.expanded_view(t, DEV), _to(DEV)
    x = synth.randn(81, (B, L, D), "o.x").to(torch.float16)
    pos = (synth.randn(82, (1, D), "o.p") * 0.1).expand(L, D).contiguous()
    gamma, beta = torch.full((D,), 1.25), torch.full((D,), -0.5)
    assert ex(pos).stride() == (0, 1) and ex(gamma).stride() == (0,) and oc.expanded_view(synth.randn(83, (D,), "o.g")) is None
    _same_bits(ops.add_pos_layernorm(dev(x), ex(pos), ex(gamma), ex(beta), want_sum=True),
               ops.add_pos_layernorm(dev(x), dev(pos), dev(gamma), dev(beta), want_sum=True), "add_pos_layernorm")
    _same_bits(ops.mean_layernorm(dev(x), ex(gamma), ex(beta)), ops.mean_layernorm(dev(x), dev(gamma), dev(beta)), "mean_layernorm")
    xf, w = synth.randn(84, (3, 8), "o.x"), synth.randn(85, (N, 8), "o.w")
    scale, shift = torch.full((N,), 0.75), torch.full((N,), 0.125)
    _same_bits(ops.linear_f32(dev(xf), dev(w), ex(scale), ex(shift), True), ops.linear_f32(dev(xf), dev(w), dev(scale), dev(shift), True), "linear_f32")
    xc, wpk = synth.randn(86, (1, 2, 2, 32), "o.x").to(torch.float16), (synth.randn(87, (N * 32 * 9,), "o.w") * 0.1).to(torch.float16)
    _same_bits(ops.conv_igemm(dev(xc), dev(wpk), ex(shift), N, 3, 1, 1, True), ops.conv_igemm(dev(xc), dev(wpk), dev(shift), N, 3, 1, 1, True),
               "conv_igemm")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. tensors the call writes
# ---------------------------------------------------------------------------------------------------------------------------------
WRITERS = [r for r in oc.ROWS if r.writes]


@pytest.mark.parametrize("row", WRITERS, ids=[r.name for r in WRITERS])
def test_a_written_tensor_is_refused_and_never_copied(row, monkeypatch):
    stub = oc.install(monkeypatch)
    values = row.build()
    for operand in row.writes:                                    # each written operand alone in aligned, non-contiguous form
        view = oc.strided_view(values[operand], DEV)
        assert view.numel() > 1 and not view.is_contiguous() and view.data_ptr() % 256 == 0
        wide_before = view._base.clone()
        with pytest.raises(ValueError) as e:
            oc.invoke(row, dict(values, **{operand: view}), _to(DEV))
        assert oc.names_operand(str(e.value), operand), (row.name, operand, str(e.value))
        torch.cuda.synchronize()
        assert guard.first_difference(view._base.cpu(), wide_before.cpu()) is None, (row.name, operand, "the caller's buffer changed")
    assert stub.calls == [], (row.name, "reached the library", [c[0] for c in stub.calls])
    monkeypatch.undo()                                            # the real library from here on
    placed = {n: (v.to(DEV, copy=True) if isinstance(v, torch.Tensor) else v) for n, v in values.items()}
    before = {n: (placed[n].data_ptr(), placed[n].clone()) for n in row.writes}
    oc.invoke(row, placed, _to(DEV))
    torch.cuda.synchronize()
    for n, (ptr, was) in before.items():
        assert placed[n].data_ptr() == ptr, (row.name, n)
        assert guard.first_difference(placed[n].cpu(), was.cpu()) is not None, (row.name, n, "the contiguous tensor was not updated in place")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. dependent operands
# ---------------------------------------------------------------------------------------------------------------------------------
PAIRS = oc.dependent_pairs()
_PAIR_NO = {(r.name, o): k + 1 for k, (r, o) in enumerate(PAIRS)}
CASES = oc.dependent_cases()
EXTRAS = [(r, e) for r in oc.ROWS for e in r.extra]


def _refused(row, operand, bad, exc, stub):
    values = row.build()
    with pytest.raises(exc) as e:
        oc.invoke(row, dict(values, **{operand: bad(values[operand]) if callable(bad) else bad}), _to(DEV))
    assert oc.names_operand(str(e.value), operand), (row.name, operand, "the message does not name the operand", str(e.value))
    assert stub.calls == [], (row.name, operand, "reached the library", [c[0] for c in stub.calls])
    with pytest.raises(oc.ReachedLibrary):                        # positive control: the valid call gets there
        oc.invoke(row, row.build(), _to(DEV))
    assert len(stub.calls) == 1, [c[0] for c in stub.calls]


@pytest.mark.parametrize("row,operand,label", CASES,
                         ids=["%s.%s[%d/%d]-%s" % (r.name, o, _PAIR_NO[(r.name, o)], len(PAIRS), lab) for r, o, lab in CASES])
def test_a_bad_dependent_operand_is_refused_before_the_library(row, operand, label, monkeypatch):
    stub = oc.install(monkeypatch)
    made = {lab: (bad, exc) for lab, bad, exc in oc.defects(row, operand, row.build()[operand])}
    bad, exc = made[label]
    _refused(row, operand, bad, exc, stub)


@pytest.mark.parametrize("row,extra", EXTRAS, ids=["%s-%s" % (r.name, e[0]) for r, e in EXTRAS])
def test_a_shape_only_the_wrapper_can_check_is_refused_before_the_library(row, extra, monkeypatch):
    """Shapes of a FREE operand that the library is never told: the `3 D` of `mha_tokens`' qkv, the rank of `match_top1`'s emb."""
    stub = oc.install(monkeypatch)
    _, operand, spoil, exc = extra
    _refused(row, operand, spoil, exc, stub)


@pytest.mark.parametrize("row", oc.ROWS, ids=[r.name for r in oc.ROWS])
def test_the_valid_call_of_every_row_reaches_the_library_once(row, monkeypatch):
    stub = oc.install(monkeypatch)
    with pytest.raises(oc.ReachedLibrary) as e:
        oc.invoke(row, row.build(), _to(DEV))
    assert [c[0] for c in stub.calls] == [e.value.entry]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. device
# ---------------------------------------------------------------------------------------------------------------------------------
def _results(row, res, placed):
    """What a call returned and what it wrote (a `MatchPack`: its buffers)."""
    if isinstance(res, ops.MatchPack):
        res = (res.packed, res.stat_w)
    return guard._flat(res) + [placed[n].cpu() for n in row.writes]


def _on_device_1(row, current):
    placed = {n: (v.to("cuda:1", copy=True) if isinstance(v, torch.Tensor) else v) for n, v in row.build().items()}
    with torch.cuda.device(current):
        res = oc.invoke(row, placed, _to("cuda:1"))
        assert torch.cuda.current_device() == current
    torch.cuda.synchronize("cuda:1")
    return _results(row, res, placed)


@pytest.mark.parametrize("row", oc.ROWS, ids=[r.name for r in oc.ROWS])
def test_operands_on_another_device_than_the_current_one(row):
    if torch.cuda.device_count() > 1:                                         # multi-GPU hosts only (as `test_configs_gpu.py`)
        ref = _on_device_1(row, 1)
        got = _on_device_1(row, 0)
        _same_bits(got, ref, row.name + " with cuda:0 current")


def test_a_prepared_gallery_on_another_device_than_the_current_one():
    if torch.cuda.device_count() > 1:                                         # multi-GPU hosts only
        G, D = 600, 64                                                        # (`test_guard_ops_gpu.py`'s packed shape)
        gal, pr = synth.unit_rows(91, G, D, "o.gal").to("cuda:1"), synth.unit_rows(92, 3, D, "o.pr").to("cuda:1")
        out = {}
        for current in (1, 0):
            with torch.cuda.device(current):
                prep = ops.match_prepare(gal)
                assert prep.packed.device == gal.device
                out[current] = [ops.match_topk(pr, gal, 5, prepared=prep), ops.match_radius(pr, 1.35, b=gal, prepared=prep),
                                ops.verify_counts(pr, torch.arange(3, dtype=torch.int32, device="cuda:1"), [0.5, 1.3], gal,
                                                  (torch.arange(G, dtype=torch.int32, device="cuda:1") % 9), prepared=prep)]
            torch.cuda.synchronize("cuda:1")
        _same_bits(out[0], out[1], "prepared gallery with cuda:0 current")
        with pytest.raises(ValueError, match="different devices"):
            ops.match_topk(pr.to("cuda:0"), gal, 5, prepared=ops.match_prepare(gal))
