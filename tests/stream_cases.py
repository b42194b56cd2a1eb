"""Stream order and graph replay: helpers of the stream tests (`test_stream_cpu.py`, `test_stream_*_gpu.py`).

A plain helper module like `guard.py` and `place_cases.py` (no fixture, no setting).  The header's contract (include/frmap_hip.h,
Conventions): the library "never allocates, frees or synchronises", its launches "are asynchronous on `stream`", and "every entry
point may be called from any host thread".  The guard tests hand a closure `run(place)` to `guard.two_fills`; here that name is one
of two further rules, and `mirror_late` / `mirror_capture` re-run a guard test - parameters, fixtures, body - under it, as
`place_cases.mirror` does for the placement rules.

THE DELAY (`delay`).  A bounded piece of device work on one stream: `torch.cuda._sleep` for a number of cycles that HIP events
calibrate once per session (a chain of device-to-device copies if `_sleep` does not behave), at most `CAP_MS` = 250 ms per call.

STALE CONTENT IS ZEROS.  An operand that is "late" holds all-zero bytes until its value arrives.  Zeros are a legal value of every
operand class of this package - floats, labels, counts, ids, boxes, images, and states ("all-zero bytes are a fresh state") - so
code that reads a stale operand still reads valid data: no rule here can turn a stream bug into an access out of bounds.  (The one
operand class zeros are NOT legal for is a threshold list, which must ascend strictly; the only wrapper that takes one checks it
on the host and refuses with `ValueError` before any launch.  A refused stale pass counts as "the values matter": not blind.)

THE LATE RULE (`late_rule`).  The reference is the eager call on the default stream.  A second eager call on zeros of the same
shapes is the blind check: if it returns the reference's bits, lateness of the operands cannot show and the call must be named in
`BLIND`.  Then two variants, each on a side stream (`side_streams`: made by `torch.cuda.Stream()` and tried once for running
beside the default stream - a fresh stream can share its hardware queue and is then served behind it), under `guard.Guard(0x5A).patch(*modules)`, each bit for bit equal to the
reference and each passing `Guard.check()`:
  (a) operands late, other streams idle: every placed operand is a zeroed buffer; the side stream gets the delay and, behind it, the
      copies of the real values.  `run` executes with the side stream current and must return to the host while the delay is still
      running.  A kernel, memset or copy that went to any other stream ran on stale operands or stale intermediates.
  (b) operands ready, default stream blocked: the delay is on the default stream, `run` and the read-back on the side stream, and the
      default stream's delay must not have finished after the read-back.  A launch that went to the default stream has not run yet:
      a final kernel whose output is still the fill, or an init / zeroing kernel that (a) cannot see because running early is
      harmless for it and running late is not.
The delay is four times the wall-clock time of the reference pass of the same closure (enqueue, synchronise, read-back: the same
host path, plus the first-call costs the timed variants no longer pay), never below a floor (four times the same measurement on
the smallest op of the guard tests, a one-element cast), never above the cap.  A variant whose "still running" assertion fails is
inconclusive: it is repeated once with the delay quadrupled (capped); inconclusive again fails the test.
A WRAPPER THAT SYNCHRONISES (`SYNCS`) cannot return while the delay runs: its host read or blocking upload waits for the stream.
For those (a) asserts instead that the delay was running when each operand was handed over; launches the wrapper makes before its
synchronisation point are still caught by (a), launches after it by (b).

THE CAPTURE RULE (`capture_rule`).  Eager references on operands A and on B = `variant(A)`; one static zeroed buffer per placed
operand; `run(place = next static buffer)` captured once on a side stream into one `torch.cuda.CUDAGraph` (one stream, no
branches); then copy A in and replay (= ref_A), copy B in and replay (= ref_B), replay untouched (= ref_B).  Catches a host read of
an operand at capture time, the address of a temporary baked into a node, a `zeros` that happened outside the captured region, and
a call that cannot be captured although the header says it can.

TABLES.  `CAPTURABLE`: every mirrored test name -> True or the wrapper line that makes the call uncapturable.  `BLIND`: calls whose
result provably does not depend on the operands' values; keys are "test", "test:what" or "test[params]:what".
"""
import contextlib
import inspect
import time

import torch

import guard

CAP_MS = 250.0
FACTOR = 4.0
FILL = 0x5A
CALLS = {"late": 0, "capture": 0}                # how often a rule ran (a mirrored test that never reaches it tests nothing)
STATS = {"max_delay_ms": 0.0, "repeats": 0, "blind": [], "late_syncing": 0, "min_lasted_ratio": float("inf")}
_CTX = {"test": None, "params": ""}              # the mirrored test now running (keys of `BLIND`, `SYNCS`, `VARIANT`)
_CAL = {}                                        # the session's calibration


# ---------------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------------
_RESIZE = "resize.py:_crop_launches / resize_bilinear_u8 build their record and tap tables on the host and upload them per call"
CAPTURABLE = {
    # test_guard_ops_gpu.py
    "test_pack_input": True, "test_normalize_u8": True, "test_maxpool": True, "test_avgpool_global": True,
    "test_avgpool_adaptive": True, "test_casts": True, "test_linear_f32_and_l2_normalize": True,
    "test_softmax_argmax_and_pairwise_distance": True, "test_gap_linear_norm": True, "test_gap_norm_match": True,
    "test_cosine_logits_and_arcmargin": True, "test_match_top1": True, "test_match_top1_empty_gallery": True,
    "test_match_topk": True,
    "test_verify_counts": "ops.verify_thresholds reads device thresholds back (`t.cpu()`) to check them on the host; it skips the "
                          "check while capturing, which `test_verify_gpu.py` covers in its own captured form",
    "test_match_radius": "ops.match_radius without capacity= reads `total.item()` between its count and its fill call",
    "test_layernorm_kernels": True, "test_mha_tokens": True, "test_cnn_attention": True, "test_track_step": True,
    "test_track_fuse": True,          # (the guard test hands `rows` over as a device tensor: nothing is uploaded)
    # test_tally_gpu.py, test_ovr_gpu.py (one test name, two modules)
    "test_guard_bands_and_placement": True,
    # test_guard_conv_gpu.py (the conv / GELU / linear cases are captured from `conv_cases.launch_case`, not mirrored: `run_case`
    # and `run_linear` read back with `.cpu()` inside the closure)
    "test_pack_conv_weight_is_guarded": True, "test_pack_conv_weight_c3_is_guarded": True,
    # test_guard_model_gpu.py
    "test_resnet_handle_forward": True, "test_resnet_handle_forward_bf16": True, "test_family_handle_forward": True,
    "test_siamese_u8_unfused_stem": True, "test_embed_and_match_and_search": True,
    # test_guard_frames_gpu.py, test_guard_yuv_gpu.py
    "test_crop_resize": _RESIZE, "test_crop_resize_tall_roi_and_batched_resize": _RESIZE, "test_align_crop": _RESIZE,
    "test_align_crop_tall_roi": _RESIZE, "test_crop_resize_yuv": _RESIZE, "test_align_crop_yuv": _RESIZE,
    "test_tall_roi_of_a_yuv_frame": _RESIZE,
}
# the wrappers of these tests synchronise their stream on the host (module docstring, "a wrapper that synchronises")
SYNCS = {name: why for name, why in CAPTURABLE.items() if why is not True}
BLIND = {
    "test_match_top1_empty_gallery": "G = 0: every probe gets -1 and inf whatever it holds",
    "test_softmax_argmax_and_pairwise_distance[B=1,C=1]:softmax_argmax": "one class: its probability is 1 and the arg-max 0",
    "test_softmax_argmax_and_pairwise_distance[B=1,C=1]:softmax_argmax pred only": "one class: the arg-max is 0",
    "test_cosine_logits_and_arcmargin[B=1,C=1,D=4]:cosine_logits argmax only": "one class: the arg-max is 0",
    "test_linear_f32_and_l2_normalize[B=1,K=4,N=1]:linear_f32": "one output behind a ReLU whose pre-activation is negative for the "
                                                                "test's operands and for their variant: 0, as for zeros (the "
                                                                "plain call of the same test, without the ReLU, is not blind)",
    "test_crop_resize_tall_roi_and_batched_resize:resize_bilinear_u8": "takes host arrays: no device operand is placed",
}


def _blind_reason(what):
    t, p = _CTX["test"], _CTX["params"]
    for key in (t, "%s:%s" % (t, what), "%s[%s]:%s" % (t, p, what)):
        if key in BLIND:
            return BLIND[key]
    return None


def _note_blind(rule, what):
    """A blind call is reported, never passed: it must be named in `BLIND`, and it is counted."""
    why = _blind_reason(what)
    label = "%s[%s]:%s" % (_CTX["test"], _CTX["params"], what)
    assert why is not None, "%s: BLIND for the %s rule - the call returns the same bits whatever its operands hold, so the rule " \
                            "cannot see it; name it in stream_cases.BLIND with the reason, or give it operands that matter" % (label, rule)
    STATS["blind"].append((rule, label, why))


# ---------------------------------------------------------------------------------------------------------------------------------
# the delay
# ---------------------------------------------------------------------------------------------------------------------------------
def _elapsed_ms(fn, stream):
    """Device time of what `fn()` enqueues on `stream`, by HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _copy_chain(n):
    a, b = _CAL["copy_bufs"]
    for _ in range(n):
        b.copy_(a)


def calibration():
    """Once per session: units (cycles of `torch.cuda._sleep`, or 64 MiB device-to-device copies) per millisecond, with a quarter
    in hand, and the proof that a requested delay lasts at least as long as asked."""
    if "per_ms" in _CAL:
        return _CAL
    s = torch.cuda.Stream()
    mode, rate = "sleep", 0.0
    try:
        torch.cuda._sleep(1000)                                     # (loads the kernel)
        torch.cuda.synchronize()
        probe = 2_000_000
        ms = min(_elapsed_ms(lambda: torch.cuda._sleep(probe), s) for _ in range(3))
        if 0.05 <= ms <= 200.0:
            rate = probe / ms
    except (RuntimeError, AttributeError):
        rate = 0.0
    if rate <= 0.0:
        mode = "copies"
        _CAL["copy_bufs"] = (torch.zeros((64 << 20,), dtype=torch.uint8, device="cuda"), torch.zeros((64 << 20,), dtype=torch.uint8, device="cuda"))
        _copy_chain(2)
        torch.cuda.synchronize()
        rate = 16 / min(_elapsed_ms(lambda: _copy_chain(16), s) for _ in range(3))
    _CAL.update(mode=mode, per_ms=rate, margin=1.25)
    for want in (2.0, 20.0):                                        # a requested delay really lasts at least as long as asked
        got = _elapsed_ms(lambda: delay(s, want), s)
        assert got >= want, "stream_cases.delay(%g ms) lasted %.3f ms (%s, %.4g units per ms)" % (want, got, mode, rate)
        _CAL["checked_%g" % want] = got
    return _CAL


def delay(stream, ms):
    """Enqueue on `stream` device work that lasts at least `ms` milliseconds, and nothing else.  A bounded spin: more than `CAP_MS`
    per call is a `ValueError`."""
    ms = float(ms)
    if not 0.0 < ms <= CAP_MS:
        raise ValueError("stream_cases.delay: %g ms is outside (0, %g]: the delay is a bounded spin" % (ms, CAP_MS))
    cal = calibration()
    units = ms * cal["per_ms"] * cal["margin"]
    with torch.cuda.stream(stream):
        if cal["mode"] == "sleep":
            torch.cuda._sleep(int(units) + 1)
        else:
            _copy_chain(int(units) + 1)


def _timed_delay(stream, ms):
    """`delay` between two timing events and followed by the event the rules query: (start, end)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        delay(stream, ms)
        e1.record()
    STATS["max_delay_ms"] = max(STATS["max_delay_ms"], ms)
    return e0, e1


def _sync():
    guard.Guard(0, 1, "cuda")._sync()


def _note_lasted(ev, ms):
    """A figure for the report, not a verdict: how long a delay lasted over what was asked (the device is synchronised).  The spin
    counts shader cycles and the clock is not constant; what the rules assert is the event query at the moment that matters."""
    STATS["min_lasted_ratio"] = min(STATS["min_lasted_ratio"], ev[0].elapsed_time(ev[1]) / ms)


_SIDE = []


def _waits_for(a, b, ms=2.0):
    """Whether work on stream `b` waits for a delay on stream `a`.  Two streams that share a hardware queue are served in order
    (a process has a handful of queues, and the default stream sits on one of them): a launch on `b` then runs behind the delay."""
    torch.cuda.synchronize()
    ev = _timed_delay(a, ms)
    with torch.cuda.stream(b):
        _CAL["probe"].add_(1)
    b.synchronize()
    waited = ev[1].query()
    torch.cuda.synchronize()
    return waited


def side_streams(n=1):
    """`n` side streams (`torch.cuda.Stream()`, made once per session, at most three) on which work runs beside a delay on the
    default stream, on each other, and the other way round.  A fresh stream can land on the default stream's hardware queue; a
    rule on such a stream is inconclusive whatever the delay, so the candidates are tried once, here, and at most eight of them."""
    assert 1 <= n <= 3
    calibration()
    if "probe" not in _CAL:
        _CAL["probe"] = torch.zeros((64,), dtype=torch.int32, device="cuda")
    tried = _CAL.setdefault("streams_tried", 0)
    while len(_SIDE) < n and tried < 8:
        s, tried = torch.cuda.Stream(), tried + 1
        if not any(_waits_for(x, s) or _waits_for(s, x) for x in [torch.cuda.default_stream()] + _SIDE):
            _SIDE.append(s)
    _CAL["streams_tried"] = tried
    assert len(_SIDE) >= n, "no %d side streams that run beside the default stream among %d candidates" % (n, tried)
    return _SIDE[:n]


def floor_ms():
    """The floor of every delay: `FACTOR` x the reference pass (enqueue, synchronise, read-back) of the smallest op of
    `test_guard_ops_gpu.py`, `test_casts` at n = 1, averaged over a few repeats after one warm call."""
    if "floor_ms" not in _CAL:
        from frmap_amd import ops, synth
        t = synth.randn(16, (1,), "g.c")

        def once():
            t0 = time.perf_counter()
            y = ops.cast_from_f32(t.to("cuda", copy=True), torch.float16)
            _sync()
            y.cpu()
            return (time.perf_counter() - t0) * 1e3
        once()
        _CAL["smallest_op_ms"] = sum(once() for _ in range(5)) / 5
        _CAL["floor_ms"] = FACTOR * _CAL["smallest_op_ms"]
    return _CAL["floor_ms"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the late rule
# ---------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return len(a) == len(b) and all(guard.first_difference(x, y) is None for x, y in zip(a, b))


def _compare(got, ref, what, how):
    assert len(got) == len(ref), (what, how, len(got), len(ref))
    for k in range(len(ref)):
        d = guard.first_difference(got[k], ref[k])
        assert d is None, "%s: result %d %s differs from the eager call on the default stream: %s" % (what, k, how, d)


def _late_a(run, modules, dev, band, canon, ms, syncing):
    """Variant (a).  Returns (conclusive, results)."""
    side, main = side_streams(1)[0], torch.cuda.default_stream()
    g = guard.Guard(FILL, band, dev)
    seen = {"ev": None, "early": False}
    staged = []                                                      # the real values, kept until `check()` has synchronised

    def place(t):
        t = t.detach().cpu().contiguous()
        with torch.cuda.stream(main):                               # the buffer and its zeros: ready before anything can read them
            a, payload = g._alloc(tuple(t.shape), t.dtype, "operand", guard._caller())
            a.cpu = t.clone()
            real = t.to(dev)
            if t.numel():
                payload.zero_()
            main.synchronize()
        with torch.cuda.stream(side):
            if seen["ev"] is None:                                   # one delay per call of the rule: later operands queue behind it
                seen["ev"], seen["t0"] = _timed_delay(side, ms), time.perf_counter()
            elif seen["ev"][1].query():
                seen["early"] = True                                 # the delay was over before this operand was handed over
            if t.numel():
                payload.copy_(real, non_blocking=True)
            staged.append(real)
        return payload

    with torch.cuda.stream(side):
        with g.patch(*modules):
            res = run(place)
        running = seen["ev"] is None or not seen["ev"][1].query()    # (no operand placed: nothing can be late)
        host_ms = (time.perf_counter() - seen["t0"]) * 1e3 if seen["ev"] is not None else 0.0
        if syncing:
            running = not seen["early"]
        got = canon(guard._flat(res))
    g.check()
    if seen["ev"] is not None:
        _note_lasted(seen["ev"], ms)
    return running, got, host_ms


def _late_b(run, modules, dev, band, canon, ms, syncing):
    """Variant (b).  Returns (conclusive, results).  Operands are placed by the guard with the side stream current: each is a
    blocking copy, ready when `place` returns."""
    side, main = side_streams(1)[0], torch.cuda.default_stream()
    g = guard.Guard(FILL, band, dev)
    _sync()
    ev, t0 = _timed_delay(main, ms), time.perf_counter()
    with torch.cuda.stream(side):
        with g.patch(*modules):
            res = run(g.place)
        got = canon(guard._flat(res))
        running = not ev[1].query()
        host_ms = (time.perf_counter() - t0) * 1e3
    g.check()
    _note_lasted(ev, ms)
    return running, got, host_ms


def until_conclusive(attempt, base_ms, what):
    """`attempt(ms)` -> (still_running, results[, host milliseconds before the query]) with `base_ms` (floored and capped); if the
    delay was over too early, once more with four times that - or eight times what the first attempt took on the host before its
    query, where that is more: the guarded pass allocates and fills bands the reference pass does not - and a failure if it was
    over too early again: an inconclusive variant has not passed.  A bounded repeat of a step that did not fault."""
    base_ms = ms = min(CAP_MS, max(base_ms, floor_ms()))
    tried = []
    for k in range(2):
        t0 = time.perf_counter()
        out = attempt(ms)
        running, got = out[0], out[1]
        if running:
            return got
        host_ms = out[2] if len(out) > 2 else (time.perf_counter() - t0) * 1e3
        tried.append("%.1f ms asked, %.1f ms on the host before the query" % (ms, host_ms))
        STATS["repeats"] += 1
        ms = min(CAP_MS, max(FACTOR * ms, 2 * FACTOR * host_ms))
    raise AssertionError("%s is INCONCLUSIVE twice: the delay was over before the call returned to the host, so nothing was late "
                         "(%s)" % (what, "; then ".join(tried)))


def reference_pass(run, dev, canon):
    """The eager call on the default stream, read back and synchronised: (flat CPU results, wall-clock milliseconds)."""
    _sync()
    t0 = time.perf_counter()
    ref = run(lambda t: t.to(dev, copy=True))
    _sync()
    ref = canon(guard._flat(ref))
    return ref, (time.perf_counter() - t0) * 1e3


LATE_VARIANTS = {"a": ("(a) operands late", _late_a), "b": ("(b) default stream blocked", _late_b)}


def late_variants(run, modules, ref, base_ms, dev, band=guard.BAND, canon=None, what="", variants=("a", "b"), syncing=False):
    """The two variants of the late rule against `ref`, from whichever host thread calls."""
    canon = canon or (lambda r: r)
    for v in variants:
        name, fn = LATE_VARIANTS[v]
        got = until_conclusive(lambda ms: fn(run, modules, dev, band, canon, ms, syncing), base_ms, "%s: variant %s" % (what, name))
        _compare(got, ref, what, "of variant " + name)


def late_rule(run, modules=(), device="cuda", band=guard.BAND, canon=None, what="", variants=("a", "b")):
    """THE LATE RULE (module docstring), with the signature of `guard.two_fills`.  Returns the eager reference as a flat list of
    CPU tensors."""
    CALLS["late"] += 1
    canon = canon or (lambda r: r)
    dev = torch.device(device)
    syncing = _CTX["test"] in SYNCS
    STATS["late_syncing"] += syncing
    ref, ref_ms = reference_pass(run, dev, canon)
    try:
        stale = canon(guard._flat(run(lambda t: torch.zeros(tuple(t.shape), dtype=t.dtype, device=dev))))
        _sync()
    except ValueError:
        stale = None                                                 # the wrapper's host check refuses zeros: the values matter
    if stale is not None and _same(stale, ref):
        _note_blind("late", what)
    late_variants(run, modules, ref, FACTOR * ref_ms, dev, band, canon, what, variants, syncing)
    return ref


# ---------------------------------------------------------------------------------------------------------------------------------
# the capture rule
# ---------------------------------------------------------------------------------------------------------------------------------
def default_variant(t, k=0):
    """Operand `t` (the k-th a call places) for the second replay: rolled by one along axis 0 where it has more than one row, so
    that all operands of a call roll together and labels stay with their rows; a one-row float is halved and rolled by k + 1 along
    its last axis (two operands of one call then differ in more than a common scale or a common permutation, which a cosine
    ignores); a one-row uint8 is 255 - v; a one-row integer is unchanged.  Deterministic; shape, dtype and - for integers - the set
    of values are kept."""
    if t.numel() == 0:
        return t.clone()
    if t.dim() >= 1 and t.shape[0] > 1:
        return torch.roll(t, 1, 0)
    if t.is_floating_point():
        h = t * 0.5
        return torch.roll(h, (k % max(t.shape[-1] - 1, 1)) + 1, -1) if t.dim() >= 2 and t.shape[-1] > 1 else h
    if t.dtype == torch.uint8:
        return 255 - t
    return t.clone()


def _scaled_variant(t, k=0):
    """Where an operand has an ordering contract (ascending thresholds; x1 <= x2, y1 <= y2 of a box): floats are halved, never
    permuted along their last axis; everything else as `default_variant`."""
    if t.is_floating_point() and t.numel():
        return torch.roll(t, 1, 0) * 0.5 if t.dim() >= 2 and t.shape[0] > 1 else t * 0.5
    return default_variant(t, k)


VARIANT = {"test_verify_counts": _scaled_variant, "test_track_step": _scaled_variant}


def variant(t, k=0, test=None):
    return VARIANT.get(test if test is not None else _CTX["test"], default_variant)(t, k)


def _flat_dev(res):
    """Returned tensors as a flat list, left on the device (None and non-tensors kept)."""
    if isinstance(res, (tuple, list)):
        out = []
        for r in res:
            out.extend(_flat_dev(r))
        return out
    return [res]


def _replaying(values, what):
    it = iter(values)

    def place(t):
        v = next(it, None)
        assert v is not None and tuple(v.shape) == tuple(t.shape) and v.dtype == t.dtype, \
            "%s: the closure places other operands than in its first pass" % what
        return v if v.is_cuda else v.to("cuda", copy=True)
    return place


def capture_rule(run, modules=(), device="cuda", band=None, canon=None, what=""):
    """THE CAPTURE RULE (module docstring), with the signature of `guard.two_fills`.  Returns the eager reference on A."""
    CALLS["capture"] += 1
    canon = canon or (lambda r: r)
    dev = torch.device(device)
    A = []

    def first(t):
        A.append(t.detach().cpu().contiguous().clone())
        return A[-1].to(dev, copy=True)
    ref_a = canon(guard._flat(run(first)))
    _sync()
    B = [variant(t, k) for k, t in enumerate(A)]
    for a, b in zip(A, B):
        assert a.shape == b.shape and a.dtype == b.dtype
    ref_b = canon(guard._flat(run(_replaying(B, what))))
    _sync()
    if _same(ref_a, ref_b):
        _note_blind("capture", what)
    static = [torch.zeros(tuple(t.shape), dtype=t.dtype, device=dev) for t in A]
    _sync()
    side, graph = side_streams(1)[0], torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            res = _flat_dev(run(_replaying(static, what)))
    _sync()
    for values, ref, how in ((A, ref_a, "of the replay on A"), (B, ref_b, "of the replay on B"), (None, ref_b, "of the second replay on B")):
        with torch.cuda.stream(side):
            for s, v in zip(static, values or ()):
                if s.numel():
                    s.copy_(v.to(dev))
            graph.replay()
        side.synchronize()
        _sync()
        got = canon(guard._flat(res))
        assert len(got) == len(ref), (what, how, len(got), len(ref))
        for k in range(len(ref)):
            d = guard.first_difference(got[k], ref[k])
            assert d is None, "%s: result %d %s differs from the eager call on the same operands: %s" % (what, k, how, d)
    return ref_a


# ---------------------------------------------------------------------------------------------------------------------------------
# mirrors
# ---------------------------------------------------------------------------------------------------------------------------------
def _param_id(fn, kwargs):
    names = [n for n in inspect.signature(fn).parameters if n in kwargs]
    return ",".join("%s=%s" % (n, kwargs[n]) for n in names if isinstance(kwargs[n], (bool, int, float, str)))


@contextlib.contextmanager
def under(rule, name, params=""):
    """Inside the block `guard.two_fills` IS `rule` ("late" or "capture") for the guard test `name`; the block must reach it."""
    fn = {"late": late_rule, "capture": capture_rule}[rule]
    assert name in CAPTURABLE, "%s is not in stream_cases.CAPTURABLE" % name
    assert rule != "capture" or CAPTURABLE[name] is True, "%s is declared uncapturable: %s" % (name, CAPTURABLE[name])
    saved, before, ctx = guard.two_fills, CALLS[rule], dict(_CTX)
    guard.two_fills = fn
    _CTX.update(test=name, params=params)
    try:
        yield
    finally:
        guard.two_fills = saved
        _CTX.update(ctx)
    assert CALLS[rule] > before, "the guard test never called guard.two_fills: the %s rule never ran" % rule


def _mirror(rule, module, name, doc):
    fn = getattr(module, name)

    def test(*args, **kwargs):
        with under(rule, name, _param_id(fn, kwargs)):
            return fn(*args, **kwargs)
    test.__name__ = test.__qualname__ = name
    test.__doc__ = doc % (module.__name__, name)
    test.__signature__ = inspect.signature(fn)
    test.pytestmark = list(getattr(fn, "pytestmark", []))
    return test


def mirror_late(module, name):
    """The guard test `module.name` under the late rule: same parameters, same fixtures, same body."""
    return _mirror("late", module, name, "`%s.%s` with its operands late, then with the default stream blocked (`late_rule`).")


def mirror_capture(module, name):
    """The guard test `module.name` captured once and replayed on changed operands (`capture_rule`)."""
    return _mirror("capture", module, name, "`%s.%s` captured into one graph and replayed on A, on B and on B again (`capture_rule`).")


def report(mirrored=()):
    """What a `test_stream_*` module prints at its end: the calibration, the largest delay, and how many calls ran under each rule,
    were blind, or are declared uncapturable (with the reasons)."""
    cal = dict(_CAL)
    cal.pop("copy_bufs", None)
    cal.pop("probe", None)
    lines = ["stream rules: %d calls under the late rule (%d of them in wrappers that synchronise), %d under the capture rule, "
             "%d inconclusive variants repeated" % (CALLS["late"], STATS["late_syncing"], CALLS["capture"], STATS["repeats"]),
             "calibration: " + ", ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in sorted(cal.items())),
             "largest delay used: %.2f ms (cap %.0f ms); shortest delay over what was asked: %.2f" % (
                 STATS["max_delay_ms"], CAP_MS, STATS["min_lasted_ratio"])]
    blind = sorted(set(STATS["blind"]))
    lines.append("blind calls: %d in %d tests" % (len(blind), len({b[1].split("[")[0] for b in blind})))
    lines += ["  blind under %s: %s (%s)" % b for b in blind]
    unc = [(n, CAPTURABLE[n]) for n in mirrored if CAPTURABLE[n] is not True]
    lines.append("uncapturable mirrored tests: %d" % len(unc))
    lines += ["  %s: %s" % u for u in unc]
    return "\n".join(lines)
