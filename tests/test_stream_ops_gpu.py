"""GPU: stream order and graph replay of the layout / pool / cast kernels, the heads, the matching entry points, the transformer
kernels, the trackers, the tally, the one-vs-rest store and the head-fitting step (`stream_cases.py`).

1. Every two-fill test of `test_guard_ops_gpu.py` (its positive control aside) and the two-fill tests of `test_tally_gpu.py` and
   `test_ovr_gpu.py` run again under the late rule - operands late on a side stream, then operands ready and the default stream
   blocked - and, where `stream_cases.CAPTURABLE` says so, captured into one graph and replayed on A, on B and on B again.  The
   head-fitting step has no two-fill test (its guard test places by hand): the same closure is written here.
2. Direct cases: a `MatchPack` that arrives late on another stream (`match_prepare`, then `update_rows`), the eager two-stream
   step of `GraphedEmbedMatch._run` with its second stream delayed, and the late rule from a host thread with a stream of its own.
3. Positive controls: an element-wise op sent to the default stream is reported by variant (a) and by variant (b); a result
   computed from a copy made before capture fails the replay on B; a call that ignores its operand is reported blind.
"""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
import fit_cases as fitc  # noqa: E402
import guard  # noqa: E402
import stream_cases as sc  # noqa: E402
import test_guard_model_gpu as tm  # noqa: E402
import test_guard_ops_gpu as tg  # noqa: E402
import test_ovr_gpu as tov  # noqa: E402
import test_tally_gpu as tta  # noqa: E402
from frmap_amd import head_fit as hf, ops, synth  # noqa: E402

DEV = "cuda"
GUARD_TESTS = [n for n in dir(tg) if n.startswith("test_") and n != "test_positive_control_one_element_too_many"]
assert len(GUARD_TESTS) >= 20
MIRRORED = list(GUARD_TESTS) + ["test_guard_bands_and_placement"]

for _name in GUARD_TESTS:
    globals()[_name + "_late"] = sc.mirror_late(tg, _name)
    if sc.CAPTURABLE[_name] is True:
        globals()[_name + "_captured"] = sc.mirror_capture(tg, _name)
for _mod, _tag in ((tta, "tally"), (tov, "ovr")):
    globals()["test_%s_guard_bands_and_placement_late" % _tag] = sc.mirror_late(_mod, "test_guard_bands_and_placement")
    globals()["test_%s_guard_bands_and_placement_captured" % _tag] = sc.mirror_capture(_mod, "test_guard_bands_and_placement")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the head-fitting step: w, b and the state are written in place, so each is a copy of its placed operand made on the call's
#    own stream (and inside the graph: a replay starts from the same weights and a fresh state)
# ---------------------------------------------------------------------------------------------------------------------------------
def _head_fit_run():
    B, D, C = 45, 70, 35
    var = fitc.variation(1 | 2 | 4 | 16)
    x, labels, w, b, rows, keep = fitc.problem(13, B, D, C)
    st = np.zeros((hf.state_bytes(D, C, True),), np.uint8)
    kw = dict(fitc.HYPER, label_smoothing=var["label_smoothing"], decoupled=var["decoupled"], amsgrad=var["amsgrad"])
    t = torch.from_numpy

    def run(place):
        xd, ld, rd, kd = place(t(x)), place(t(labels)), place(t(rows)), place(t(keep))
        wd, bd, sd = place(t(w)).clone(), place(t(b)).clone(), place(t(st)).clone()
        wsd = torch.empty((hf.workspace_bytes(B, D, C),), dtype=torch.uint8, device=DEV)
        hf.step(xd, ld, wd, bd, sd, wsd, rd, kd, 1.0 / 0.75, **kw)
        return wd, bd, sd, wsd
    return run


def test_head_fit_step_late():
    sc.late_rule(_head_fit_run(), [hf], what="head_fit.step")


def test_head_fit_step_captured():
    sc.capture_rule(_head_fit_run(), [hf], what="head_fit.step")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. direct cases
# ---------------------------------------------------------------------------------------------------------------------------------
PACK_G, PACK_D, PACK_B = 512, 32, 3            # the smallest gallery that takes the packed path (`ops.wants_pack`)


def _flat(res):
    return guard._flat(res)


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k in range(len(want)):
        d = guard.first_difference(got[k], want[k])
        assert d is None, "%s: result %d differs from the eager call: %s" % (what, k, d)


def test_a_pack_that_arrives_late_on_another_stream_is_waited_for():
    """Stream A: delay, the gallery's rows, `match_prepare`.  Stream B, with no wait of its own: `match_top1` and `match_topk` on
    that pack.  `MatchPack.wait_ready` is the only thing that orders B after A."""
    G, D, B = PACK_G, PACK_D, PACK_B
    assert ops.wants_pack(G, D) and not ops.wants_pack(G - 1, D)
    gal, pr = synth.unit_rows(71, G, D, "s.gal"), synth.unit_rows(72, B, D, "s.pr")
    pr[0] = gal[G // 2]
    prd = pr.to(DEV)

    def eager(place):
        g = place(gal)
        pack = ops.match_prepare(g)
        return ops.match_top1(prd, g, 0.9, packed=True, prepared=pack), ops.match_topk(prd, g, 5, prepared=pack)
    want, ref_ms = sc.reference_pass(eager, torch.device(DEV), lambda r: r)
    assert int(want[0][0]) == G // 2

    def attempt(ms):
        a, b = sc.side_streams(2)
        gd, real = torch.zeros((G, D), device=DEV), gal.to(DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(a):
            ev = sc._timed_delay(a, ms)
            gd.copy_(real, non_blocking=True)
            pack = ops.match_prepare(gd)
        with torch.cuda.stream(b):
            res = ops.match_top1(prd, gd, 0.9, packed=True, prepared=pack), ops.match_topk(prd, gd, 5, prepared=pack)
            running = not ev[1].query()
            got = _flat(res)
        torch.cuda.synchronize()
        return running, got
    _same(sc.until_conclusive(attempt, sc.FACTOR * ref_ms, "late pack"), want, "match on a late pack")


def test_rows_appended_late_on_another_stream_are_waited_for():
    """`MatchPack.update_rows` on stream A behind a delay; the match against the grown gallery on stream B."""
    G, D, B, more = PACK_G, PACK_D, PACK_B, 70
    rows = synth.unit_rows(73, G + more, D, "s.gal")
    pr = synth.unit_rows(74, B, D, "s.pr")
    pr[0], pr[1] = rows[G // 2], rows[G + 5]                          # one probe is a late row
    prd = pr.to(DEV)

    def eager(place):
        g = place(rows)
        pack = ops.match_prepare(g)
        return ops.match_top1(prd, g, 0.9, packed=True, prepared=pack), ops.match_topk(prd, g, 5, prepared=pack)
    want, ref_ms = sc.reference_pass(eager, torch.device(DEV), lambda r: r)
    assert want[0][:2].tolist() == [G // 2, G + 5]

    def attempt(ms):
        a, b = sc.side_streams(2)
        store, late = torch.zeros((G + more, D), device=DEV), rows[G:].to(DEV)
        store[:G] = rows[:G].to(DEV)
        with torch.cuda.stream(a):
            pack = ops.MatchPack(store[:G], capacity=G + more)
        torch.cuda.synchronize()
        with torch.cuda.stream(a):
            ev = sc._timed_delay(a, ms)
            store[G:].copy_(late, non_blocking=True)
            grown = store[:G + more]
            pack.update_rows(grown, G, G + more)
        with torch.cuda.stream(b):
            res = ops.match_top1(prd, grown, 0.9, packed=True, prepared=pack), ops.match_topk(prd, grown, 5, prepared=pack)
            running = not ev[1].query()
            got = _flat(res)
        torch.cuda.synchronize()
        return running, got
    _same(sc.until_conclusive(attempt, sc.FACTOR * ref_ms, "late rows"), want, "match on late rows")


def test_the_eager_two_stream_step_with_its_second_stream_delayed(calibrated_sd):
    """What `GraphedEmbedMatch._run` does outside a graph: two micro-batches of a model handle write their slices of one record
    buffer, the second on a stream of its own that forks from and joins the first.  The second stream is delayed before its half.
    The reference is the same two calls on one stream (a micro-batch plans its own kernels: the whole batch in one call is another
    sum order, which `test_bench_gpu.py` bounds)."""
    mt, B, HW = tm.MATCH_MODELS[0]
    h = tm._handle(calibrated_sd, mt)
    G, D = 600, h.embedding_dim
    x = tm._input(95, B, HW, HW, False).to(DEV)
    gal = synth.unit_rows(96, G, D, "s.gal").to(DEV)
    pack = ops.match_prepare(gal)
    xs = list(x.chunk(2))
    cuts = [0, xs[0].shape[0], B]
    torch.cuda.synchronize()

    def one_stream(place):
        rec = torch.full((B, 2), -7, dtype=torch.int32, device=DEV)
        for k in range(2):
            h.embed_and_match(xs[k], gal, pack, 1.1, False, packed=rec[cuts[k]:cuts[k + 1]])
        return rec
    want, ref_ms = sc.reference_pass(one_stream, torch.device(DEV), lambda r: r)

    def attempt(ms):
        main, second = sc.side_streams(2)
        with torch.cuda.stream(main):
            rec = torch.full((B, 2), -7, dtype=torch.int32, device=DEV)
            second.wait_stream(main)
            with torch.cuda.stream(second):
                ev = sc._timed_delay(second, ms)
                h.embed_and_match(xs[1], gal, pack, 1.1, False, packed=rec[cuts[1]:cuts[2]])
            h.embed_and_match(xs[0], gal, pack, 1.1, False, packed=rec[cuts[0]:cuts[1]])
            main.wait_stream(second)
            running = not ev[1].query()
            got = _flat(rec)
        torch.cuda.synchronize()
        return running, got
    _same(sc.until_conclusive(attempt, sc.FACTOR * ref_ms, "two-stream step"), want, "the two-stream step")


def _conv_run():
    case, dtype = cc.CONV_CASES[0], torch.float16
    o = cc.gpu_operands(case, "exact", dtype)
    return lambda place: cc.launch_case(case, cc.device_operands(case, o, dtype, place), dtype, sync=False)


def _top1_run():
    gal, pr = tg._gallery_and_probes(1, 65, 41)
    return lambda place: ops.match_top1(place(pr), place(gal), 0.9, packed=True)


@pytest.mark.parametrize("make", [_conv_run, _top1_run], ids=["conv", "match_top1"])
def test_the_late_rule_from_a_host_thread_with_a_stream_of_its_own(make):
    """ "Every entry point may be called from any host thread": torch's current stream is per thread, so the wrappers must read it in
    the thread that calls them.  Both variants run in a `threading.Thread`; in (b) the stream that is blocked is the main thread's."""
    run, dev = make(), torch.device(DEV)
    ref, ref_ms = sc.reference_pass(run, dev, lambda r: r)
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    box = []

    def work():
        try:
            sc.late_variants(run, [ops], ref, sc.FACTOR * ref_ms, dev, what="from a thread")
            box.append(None)
        except BaseException as e:                                   # (handed to the main thread)
            box.append(e)
    t = threading.Thread(target=work)
    t.start()
    t.join()
    torch.cuda.synchronize()
    assert box and box[0] is None, box


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. positive controls: element-wise, every access inside its own buffers; what is read too early is zeros or the fill
# ---------------------------------------------------------------------------------------------------------------------------------
def _on_the_default_stream(x):
    """A wrapper with the bug the late rule is for: its launch goes to the default stream, whatever stream is current."""
    with torch.cuda.stream(torch.cuda.default_stream()):
        return ops.l2_normalize(x)


@pytest.mark.parametrize("v", ["a", "b"])
def test_positive_control_a_launch_on_the_default_stream_is_reported(v):
    x = synth.randn(81 + ord(v), (3, 64), "s.x")
    with pytest.raises(AssertionError, match="differs from the eager call on the default stream"):
        sc.late_rule(lambda place: _on_the_default_stream(place(x)), [ops], what="control", variants=(v,))
    torch.cuda.synchronize()
    # (other values: in (b) the misdirected output is read before anything wrote it, and a recycled block must not hold this answer)
    x2 = synth.randn(85 + ord(v), (3, 64), "s.x")
    sc.late_rule(lambda place: ops.l2_normalize(place(x2)), [ops], what="control without the stream context", variants=(v,))


def test_positive_control_a_copy_made_before_capture_fails_the_replay_on_b():
    x = synth.randn(82, (3, 64), "s.x")
    snap = []

    def run(place):
        xd = place(x)
        if not snap:
            snap.append(xd.clone())                                  # (the first eager pass: operand A, outside any capture)
        return ops.l2_normalize(snap[0] if torch.cuda.is_current_stream_capturing() else xd)
    with pytest.raises(AssertionError, match="of the replay on B differs"):
        sc.capture_rule(run, [ops], what="control")
    torch.cuda.synchronize()
    sc.capture_rule(lambda place: ops.l2_normalize(place(x)), [ops], what="control without the copy")


@pytest.mark.parametrize("rule", [sc.late_rule, sc.capture_rule], ids=["late", "capture"])
def test_positive_control_a_call_that_ignores_its_operand_is_blind_not_passed(rule):
    x = synth.randn(83, (3, 64), "s.x")
    const = synth.randn(84, (3, 64), "s.c").to(DEV)
    before = len(sc.STATS["blind"])
    with pytest.raises(AssertionError, match="BLIND"):
        rule(lambda place: (place(x), ops.l2_normalize(const))[1], [ops], what="control")
    assert len(sc.STATS["blind"]) == before


def test_stream_report(capsys):
    assert sc.CALLS["late"] > 0 and sc.CALLS["capture"] > 0
    with capsys.disabled():
        print("\n[test_stream_ops_gpu] " + sc.report(MIRRORED))
