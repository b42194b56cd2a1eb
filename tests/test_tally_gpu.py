"""GPU: the classification tally kernel (`ops.classify_tally`, csrc/classify_tally.hip) against the rule of `evaluate.tally_rule`.

* Shapes C in {1, 2, 36, 63, 64, 65, 129, 1000} x B in {1, 5, 259} on the rows of `tally_cases.gpu_rows` (the +-80 row, the ties
  inside a lane and across lanes, the target tied with the maximum at a higher index): pred and rank equal the numpy rule
  exactly; conf is within 1e-6 absolute of float64; loss is gated at 4x a CPU measurement - the worst deviation from float64 of
  a numpy fp32 restatement of the kernel's summation order over the case's own rows, floor 2^-22 (every figure is printed;
  the worst of each over all cases, measured on an MI355X, is in DESIGN.md section 4, "Classification tally"); the state
  equals the host twin's on the device's own row records, word for word; no confidence of the float64 reference is a knife edge.
* Declined rows, carry and order across launches, the options, contention on one class, guard bands and placement at element
  alignment, one case past 2^31 logits, a captured graph, and `evaluate_stream` against `evaluate_model`.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import big_cases as bc  # noqa: E402
import guard  # noqa: E402
import tally_cases as tc  # noqa: E402
import frmap_amd  # noqa: E402
from frmap_amd import evaluate, ops  # noqa: E402

DEV = "cuda"
F32 = np.float32


def _run(z, y, state=None, confusion=True, want_rows=True, ranks=tc.RANKS, n_bins=tc.N_BINS):
    out = ops.classify_tally(tc.t(z).to(DEV), tc.t(y).to(DEV), state, ranks, n_bins, confusion, want_rows)
    torch.cuda.synchronize()
    if not want_rows:
        return out.cpu().numpy().view(np.uint64), None
    st, rows = out
    return st.cpu().numpy().view(np.uint64), tuple(r.cpu().numpy() for r in rows)


@pytest.mark.parametrize("B", tc.GPU_B)
@pytest.mark.parametrize("C", tc.GPU_C)
def test_rows_and_state_against_the_rule(C, B):
    z_all, y_all, ref_all = tc.gpu_rows(C)
    z, y = z_all[:B], y_all[:B]
    pred64, rank64, conf64, loss64 = (a[:B] for a in ref_all)
    gap = tc.assert_no_knife_edge(conf64)                                   # every row, from the float64 reference
    state, (pred, rank, conf, loss) = _run(z, y)
    assert np.array_equal(pred, pred64) and np.array_equal(rank, rank64)    # exact integers
    assert conf.dtype == F32 and loss.dtype == F32
    conf_err = float(np.abs(conf.astype(np.float64) - conf64).max())
    # the loss gate: 4 x the worst deviation from float64 of the kernel's summation order restated in numpy fp32, measured here on
    # the CPU over this case's own rows; floor 2^-22
    _, loss_cpu = tc.kernel_order_rows(z, y)
    cpu_dev = float(np.abs(loss_cpu.astype(np.float64) - loss64).max())
    gate = max(4.0 * cpu_dev, tc.LOSS_FLOOR)
    loss_err = float(np.abs(loss.astype(np.float64) - loss64).max())
    print("\ntally C=%d B=%d: conf err %.3g | loss err %.3g, numpy fp32 restatement %.3g, gate %.3g | nearest bin edge %.3g"
          % (C, B, conf_err, loss_err, cpu_dev, gate, gap))
    assert conf_err <= 1e-6, conf_err
    assert loss_err <= gate, (loss_err, cpu_dev, gate)
    # the state: the host twin on the device's own row records, word for word - and the numpy rule
    twin, p2, r2 = ops.classify_tally_host(z, y, conf, loss)
    assert np.array_equal(p2, pred) and np.array_equal(r2, rank)
    assert np.array_equal(state, twin), np.nonzero(state != twin)[0][:8]
    assert np.array_equal(state, evaluate.tally_rule(z, y, conf, loss)[0])
    assert int(state[0]) == B and int(state[1]) == 0 and int(state[2]) == 0 and not state[5:8].any()
    if B >= 5 and C >= 2:
        assert pred[1] == 0 and rank[1] == 0 and pred[4] == 0 and rank[4] == 1
    if B >= 5 and C > 65:
        assert (pred[2], rank[2], pred[3], rank[3]) == (0, 1, 63, 1)


def test_declined_rows_add_only_their_counter():
    C = 36
    z0, y0, _ = tc.gpu_rows(C)
    z0, y0 = z0[:40], y0[:40]
    base, _ = _run(z0, y0)
    extra = np.zeros((5, C), F32)
    extra[2, 7], extra[3, 35], extra[4, 0] = np.nan, np.inf, -np.inf
    extra[0, :] = 9.0                                                       # label -1: ignored whatever the logits are
    ye = np.array([-1, C, 3, 3, 3], np.int32)
    at = [0, 7, 20, 33, 40]                                                 # where the declined rows go in
    z, y = np.insert(z0, at, extra, axis=0), np.insert(y0, at, ye)
    where = np.array([a + k for k, a in enumerate(at)])
    state, (pred, rank, conf, loss) = _run(z, y)
    assert int(state[1]) == 2 and int(state[2]) == 3 and int(state[0]) == 40
    assert (pred[where] == -1).all() and (rank[where] == -1).all() and np.isnan(conf[where]).all() and np.isnan(loss[where]).all()
    keep = np.ones(len(y), bool)
    keep[where] = False
    assert (pred[keep] >= 0).all() and not np.isnan(conf[keep]).any()
    other = np.ones(len(state), bool)
    other[1:3] = False
    assert np.array_equal(state[other], base[other])                        # no other word differs


def test_carry_order_and_repeat_are_bit_for_bit():
    C = 65
    z, y, _ = tc.gpu_rows(C)
    once, rows = _run(z, y)
    again, rows2 = _run(z, y)
    assert np.array_equal(once, again) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(rows, rows2))
    st = None
    for lo, hi in zip((0,) + tc.SPLIT, tc.SPLIT + (tc.B_FULL,)):
        st = ops.classify_tally(tc.t(z[lo:hi]).to(DEV), tc.t(y[lo:hi]).to(DEV), st)
    assert np.array_equal(st.cpu().numpy().view(np.uint64), once)
    back, _ = _run(z[::-1].copy(), y[::-1].copy())
    assert np.array_equal(back, once)


def test_options_leave_the_counts_alone():
    C = 36
    z, y, _ = tc.gpu_rows(C)
    kept, _ = _run(z, y)
    without, _ = _run(z, y, confusion=False)
    lay = ops.classify_tally_layout(C, tc.RANKS, tc.N_BINS, True)
    assert lay["confusion"].stop == len(kept) and np.array_equal(without, kept[:lay["confusion"].start])
    no_rows, none = _run(z, y, want_rows=False)
    assert none is None and np.array_equal(no_rows, kept)
    # a non-contiguous operand is copied, not misread
    wide = torch.zeros((tc.B_FULL, 2 * C), dtype=torch.float32, device=DEV)
    wide[:, ::2] = tc.t(z).to(DEV)
    st = ops.classify_tally(wide[:, ::2], tc.t(y).to(DEV))
    assert np.array_equal(st.cpu().numpy().view(np.uint64), kept)
    with pytest.raises(ValueError, match="state holds"):
        ops.classify_tally(tc.t(z).to(DEV), tc.t(y).to(DEV), torch.zeros(5, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        ops.classify_tally(tc.t(z), tc.t(y))                                # host tensors: no CPU fallback


def test_contention_on_one_class_is_exact():
    B = 4096
    z = np.tile(np.array([[1.5, -0.5]], F32), (B, 1))
    y = np.zeros(B, np.int32)
    state, (pred, rank, conf, loss) = _run(z, y)
    c = evaluate.tally_counts(state, 2)
    assert c["rows"] == B and c["correct"] == B and c["ignored"] == 0 and c["nonfinite"] == 0
    assert c["support"].tolist() == [B, 0] and c["predicted"].tolist() == [B, 0] and c["hit"].tolist() == [B, 0]
    assert c["rank_hist"].tolist() == [B, 0, 0, 0, 0, 0] and c["confusion"].tolist() == [[B, 0], [0, 0]]
    assert (conf == conf[0]).all() and (loss == loss[0]).all() and (pred == 0).all() and (rank == 0).all()
    b = int(np.digitize(float(conf[0]), evaluate.tally_edges(10))) - 1
    assert c["bin_count"][b] == B and c["bin_correct"][b] == B and int(c["bin_conf_q"][b]) == B * int(np.rint(float(conf[0]) * 2.0 ** 32))
    assert c["loss_q"] == B * int(np.rint(float(loss[0]) * 2.0 ** 24))


@pytest.mark.parametrize("C,B", [(65, 37), (1000, 5)])
def test_guard_bands_and_placement(C, B):
    z_all, y_all, _ = tc.gpu_rows(C)
    z, y = tc.t(z_all[:B]), tc.t(y_all[:B])
    run = lambda place: ops.classify_tally(place(z), place(y), None, want_rows=True)
    # logits and labels placed, the state and the four row outputs allocated by the wrapper: all between bands, fills 0xFF and 0x5A
    ref = guard.two_fills(run, [ops], what="classify_tally")
    assert len(ref) == 5 and ref[0].dtype == torch.int64 and int(ref[0][0]) == B
    # every buffer aligned to its element size and not to twice it
    elem = lambda dtype, kind, who: torch.empty((), dtype=dtype).element_size()
    again = guard.shifted(run, [ops], what="classify_tally at element alignment", requirement=elem)
    assert all(guard.first_difference(a, b) is None for a, b in zip(ref, again))


def test_logits_past_two_to_the_31_elements():
    """B * C just past 2^31 logits (and 8 GiB): zero logits on the device, label = row % C, so pred = 0, rank = label and
    conf = 1 / C for every row but the last three, which get values of their own."""
    C, B = 33, 2 ** 26 - 4                                                   # the launcher's largest batch
    assert B * C > 2 ** 31 and B * C * 4 > 2 ** 32 and B == bc.WAVE_ROWS_LIMIT - 1
    # logits, the bool temporary of the intact check, two int64 temporaries of the labels, labels, the four row outputs
    bc.need_memory(bc.estimate_bytes([B * C * 4, B * C, 2 * B * 8, B * 4, 4 * B * 4]), "classify_tally-big")
    logits = labels = rows = state = None
    try:
        logits = torch.zeros((B, C), dtype=torch.float32, device=DEV)
        labels = (torch.arange(B, device=DEV) % C).to(torch.int32)
        tail = np.zeros((3, C), F32)
        tail[0, 0], tail[1, 32], tail[2, 7] = -2.0, 3.0, 5.0                 # pred 1, 32, 7
        logits[B - 3:] = tc.t(tail).to(DEV)
        state, rows = ops.classify_tally(logits, labels, want_rows=True)
        torch.cuda.synchronize()
        pred, rank, conf, loss = rows
        n = B - 3
        assert bool((pred[:n] == 0).all()) and bool((rank[:n] == labels[:n]).all())
        assert bool((conf[:n] == conf[0]).all()) and bool((loss[:n] == loss[0]).all())
        assert abs(float(conf[0]) - 1.0 / C) < 1e-7 and abs(float(loss[0]) - np.log(C)) < 1e-6
        far_y = labels[n:].cpu().numpy()
        p64, r64, c64, l64 = evaluate.tally_rows_reference(tail, far_y)
        assert pred[n:].cpu().tolist() == p64.tolist() == [1, 32, 7] and rank[n:].cpu().tolist() == r64.tolist()
        assert np.abs(conf[n:].cpu().numpy() - c64).max() < 1e-6 and np.abs(loss[n:].cpu().numpy() - l64).max() < 1e-5
        # the integer totals: the first n rows analytically, the far rows by the rule
        conf0, loss0 = conf[:1].cpu().numpy(), loss[:1].cpu().numpy()
        want = evaluate.tally_rule(tail, far_y, conf[n:].cpu().numpy(), loss[n:].cpu().numpy())[0]
        lay = evaluate.tally_layout(C, tc.RANKS, tc.N_BINS, True)
        per_class = np.array([n // C + (1 if c < n % C else 0) for c in range(C)], np.uint64)
        want[0] += np.uint64(n)
        want[3] += per_class[0]
        want[4] += np.uint64(n * int(np.rint(float(loss0[0]) * 2.0 ** 24)))
        hist = np.concatenate([per_class[:tc.RANKS - 1], [per_class[tc.RANKS - 1:].sum()]]).astype(np.uint64)
        want[lay["rank_hist"]] += hist
        want[lay["support"]] += per_class
        want[lay["predicted"].start] += np.uint64(n)
        want[lay["hit"].start] += per_class[0]
        b = int(np.digitize(float(conf0[0]), evaluate.tally_edges(tc.N_BINS))) - 1
        want[lay["bin_count"].start + b] += np.uint64(n)
        want[lay["bin_correct"].start + b] += per_class[0]
        want[lay["bin_conf_q"].start + b] += np.uint64(n * int(np.rint(float(conf0[0]) * 2.0 ** 32)))
        want[lay["confusion"].start + np.arange(C) * C] += per_class
        got = state.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
        assert bool((logits[:n] == 0).all())                                 # the operand is intact
    finally:
        del logits, labels, rows, state
        bc.release()


def test_a_captured_update_replayed_twice_adds_twice():
    C = 129
    z, y, _ = tc.gpu_rows(C)
    zd, yd = tc.t(z).to(DEV), tc.t(y).to(DEV)
    single = evaluate.ClassificationTally(C).update(zd, yd).counts()
    tally = evaluate.ClassificationTally(C)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tally.update(zd, yd)                                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    tally.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tally.update(zd, yd)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    twice = tally.counts()
    for name, v in single.items():
        assert np.array_equal(np.asarray(twice[name]), 2 * np.asarray(v)), name
    # merge: the integer add of two tallies is the tally of both
    merged = evaluate.ClassificationTally(C).update(zd[:100], yd[:100]).merge(evaluate.ClassificationTally(C).update(zd[100:], yd[100:]))
    assert all(np.array_equal(np.asarray(merged.counts()[k]), np.asarray(v)) for k, v in single.items())
    assert evaluate.ClassificationTally(C).update(zd[:0], yd[:0]).counts()["rows"] == 0     # an empty batch is a no-op


@pytest.mark.parametrize("mt", ["cnn", "arcface"])
def test_evaluate_stream_against_evaluate_model(mt, calibrated_sd):
    from sklearn.metrics import confusion_matrix
    from frmap_amd import synth
    m = frmap_amd.get_model(mt, 36)
    m.load_state_dict(calibrated_sd(mt))
    m = m.to(DEV).eval().set_compute_dtype(torch.float16)
    n = 75                                                                   # batches of 32, 32 and 11
    x = synth.randn(77, (n, 3, 64, 64), "tally-eval")
    lab = torch.from_numpy(np.random.default_rng(78).integers(0, 36, n))
    batches = [(x[lo:lo + 32], lab[lo:lo + 32]) for lo in range(0, n, 32)]
    res = evaluate.evaluate_model(m, mt, batches)
    got = evaluate.evaluate_stream(m, mt, batches)
    assert got["rows"] == n and got["ignored"] == 0 and got["nonfinite"] == 0
    for k in ("accuracy", "precision", "recall", "f1"):
        assert abs(got[k] - res["metrics"][k]) <= 1e-12, (k, got[k], res["metrics"][k])
    want = confusion_matrix(res["targets"], res["predictions"], labels=list(range(36)))
    assert np.array_equal(np.array(got["confusion"]["matrix"]), want)
    # the loss is the per-sample mean: -log of evaluate_model's own fp32 probability of the target (relative error of a few
    # 2^-24 each, so a few 1e-6 on the loss); its `test_loss`, the mean of three batch means with a short last batch, is another number
    per = -np.log(np.array(res["probabilities"])[np.arange(n), np.array(res["targets"])])
    print("\nevaluate_stream %s: loss %.6f, per-sample mean of evaluate_model's probabilities %.6f, its mean of batch means %.6f, accuracy %.3f"
          % (mt, got["loss"], per.mean(), res["test_loss"], got["accuracy"]))
    assert np.isfinite(per).all() and abs(got["loss"] - per.mean()) <= 1e-4 * max(1.0, per.mean())
    assert "roc_auc" not in got and got["calibration"]["n_bins"] == 10 and sum(got["calibration"]["bin_counts"]) == n
    with pytest.raises(ValueError, match="siamese"):
        evaluate.evaluate_stream(m, "siamese", batches)
