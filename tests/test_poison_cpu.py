"""CPU: the rules of `poison.py` on hand-made "kernel outputs", the way `test_guard_cpu.py` treats the guard bands.

The operation is relu(conv 1x3, pad 1) along W on a [3, 2, 1, 6] input, fp16 storage, no zero weight; the "kernel" is the float64
reference rounded to fp16, which passes; each negative case then damages ONE element of the poisoned output the way a kernel
could, and `compare()` must name the rule and the element.  Each of the four negative cases was seen to fail once with its
check line in `poison.compare` disabled.
"""
import math

import pytest
import torch

import poison

W3 = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)


def _op(x):
    """float64 relu(sum_k x[.., w + k - 1] W3[k]) with zero padding, every channel on its own."""
    xp = torch.zeros(x.shape[:-1] + (x.shape[-1] + 2,), dtype=torch.float64)
    xp[..., 1:-1] = x.double()
    return (xp[..., :-2] * W3[0] + xp[..., 1:-1] * W3[1] + xp[..., 2:] * W3[2]).clamp_min(0)


def _setup(kind, index=(1, 0, 0, 2)):
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 2, 1, 6), generator=g).half()
    xp = poison.poisoned(x, index, poison.poison_value(kind))
    ref_c, ref_p = _op(x), _op(xp)
    foot = poison.nan_footprint(_op(poison.poisoned(x, index, math.nan)))
    return ref_c.half(), ref_p.half(), ref_c, ref_p, foot, index


def test_classifier_and_positions():
    t = torch.tensor([math.nan, math.inf, -math.inf, 0.0, -65504.0], dtype=torch.float16)
    assert poison.classify(t).tolist() == [poison.NAN, poison.PINF, poison.NINF, poison.FINITE, poison.FINITE]
    pos = dict(poison.positions((4, 8, 5, 6)))
    assert pos["first"] == (0, 0, 0, 0) and pos["last"] == (3, 7, 4, 5)
    assert pos["img0-last-row"][0] == 0 and pos["img0-last-row"][2] == 4 and pos["img1-first-row"][0] == 1 and pos["img1-first-row"][2] == 0
    assert pos["centre"][0] == 2 and {p[1] for p in pos.values()} >= {0, 7}                   # first and last channel
    assert len(poison.positions((1, 2, 1, 1))) == 2 and[n for n, _ in poison.positions((5, 7))] == ["first", "last", "row0-end", "row1-start", "centre"]


@pytest.mark.parametrize("kind", poison.KINDS)
def test_faithful_output_passes(kind):
    got_c, got_p, ref_c, ref_p, foot, idx = _setup(kind)
    assert int(foot.sum()) == 3 and bool(foot[1, 0, 0, 1:4].all())
    poison.compare(got_c, got_p, ref_c, ref_p, foot, image=idx[0], what=kind)
    if kind == "-inf":         # the tap with the negative weight gives +inf, the others relu(-inf) = 0 exactly
        assert poison.classify(got_p[1, 0, 0, 1:4]).tolist() == [poison.FINITE, poison.PINF, poison.FINITE] and float(got_p[1, 0, 0, 1]) == 0.0


def test_swallowed_nan_is_rule_1():
    got_c, got_p, ref_c, ref_p, foot, idx = _setup("nan")
    got_p[1, 0, 0, 2] = 0.0                                                # fmaxf(NaN, 0)
    with pytest.raises(poison.PoisonError) as e:
        poison.compare(got_c, got_p, ref_c, ref_p, foot, image=1, what="x (1,0,0,2) nan")
    assert e.value.rule == 1 and e.value.index == (1, 0, 0, 2) and "x (1,0,0,2) nan" in str(e.value)


def test_wrong_finite_is_rule_2():
    got_c, got_p, ref_c, ref_p, foot, idx = _setup("-inf")
    assert float(ref_c[1, 0, 0, 1]) > 0 and float(ref_p[1, 0, 0, 1]) == 0        # relu(-inf): changed, finite
    got_p[1, 0, 0, 1] = got_c[1, 0, 0, 1]                                   # the clean value survives where 0 is due
    with pytest.raises(poison.PoisonError) as e:
        poison.compare(got_c, got_p, ref_c, ref_p, foot, image=1)
    assert e.value.rule == 2 and e.value.index == (1, 0, 0, 1)


def test_other_image_is_rule_3():
    got_c, got_p, ref_c, ref_p, foot, idx = _setup("+inf")
    got_p[2, 1, 0, 0] = (got_p[2, 1, 0, 0].view(torch.int16) ^ 1).view(torch.float16)     # one bit of image 2
    halo = torch.ones_like(foot)                                           # even a halo over everything does not excuse it
    with pytest.raises(poison.PoisonError) as e:
        poison.compare(got_c, got_p, ref_c, ref_p, foot, image=1, halo=halo)
    assert e.value.rule == 3 and e.value.index == (2, 1, 0, 0)


def test_outside_declared_halo_is_rule_4():
    got_c, got_p, ref_c, ref_p, foot, idx = _setup("+inf")
    halo = torch.zeros_like(foot)
    halo[1, 0, 0, 0] = True                                                # the declared halo: a pad tap two columns to the left
    got_p[1, 0, 0, 0] = math.nan
    poison.compare(got_c, got_p, ref_c, ref_p, foot, image=1, halo=halo)   # NaN inside the halo: tolerated
    got_p[1, 0, 0, 4] = math.nan                                           # the same on the other side: not declared
    with pytest.raises(poison.PoisonError) as e:
        poison.compare(got_c, got_p, ref_c, ref_p, foot, image=1, halo=halo)
    assert e.value.rule == 4 and e.value.index == (1, 0, 0, 4)
    got_p[1, 0, 0, 4] = got_c[1, 0, 0, 4]
    got_p[1, 0, 0, 0] = got_c[1, 0, 0, 0] + 1                              # inside the halo, finite and different: never
    with pytest.raises(poison.PoisonError) as e:
        poison.compare(got_c, got_p, ref_c, ref_p, foot, image=1, halo=halo)
    assert e.value.rule == 2 and e.value.index == (1, 0, 0, 0)


def test_case_conditions():
    poison.assert_no_zero(W3)
    with pytest.raises(AssertionError):
        poison.assert_no_zero(torch.tensor([1.0, 0.0]))
    poison.assert_fp32_safe(torch.tensor([1e10, math.inf]))
    with pytest.raises(AssertionError):
        poison.assert_fp32_safe(torch.tensor([1e35]))
    poison.overflow_ok(torch.tensor([3.0e5, -100.0, 3.0e4]))
    with pytest.raises(AssertionError):
        poison.overflow_ok(torch.tensor([7.0e4, 1.0]))                      # fp32 order could decide the class
    with pytest.raises(AssertionError):
        poison.overflow_ok(torch.tensor([1.0, 2.0]))                        # nothing overflows
