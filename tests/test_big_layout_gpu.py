"""GPU: the layout, pool, cast, token and head kernels on tensors past the 2 GiB and 4 GiB offset marks (`big_cases.py`: periodic
operands of period 7, `big_cases.run_periodic`).

`pack_input` (both kernels) and its uint8 twin `normalize_u8`, `cast_to_f32`, `cast_from_f32`, `maxpool`, `avgpool_global`,
`avgpool_adaptive`, the token kernels of transformer.hip (`add_pos_layernorm` just under its rows < 2^31 / 64 limit on the scalar
path and past 4 GiB on the 16-byte path, `mha_tokens`, `mean_layernorm`, `cnn_attention`), `l2_normalize` and `pairwise_distance`
at B D > 2^31, `linear_f32` at the largest row count of its grid.  Every large operand and output passes 2^32 bytes and 2^31
elements (fp32: 8 GiB) by two periods, an output of a few bytes per item excepted (`pairwise_distance`'s; `avgpool_global`'s, whose
launcher takes at most 2^26 - 4 waves: a grid of 2^32 threads or more is cut down without an error, which the first run of this
file found - the case's first form launched 2^34 + 1024 threads and 1,024 of them ran).  Items are small, so the row, wave and
workgroup counts are large: every case stays under the launchers' grid limits (`big_cases.BIG_LAYOUT`).

Per case: the op on the 7-item block passes the acceptance rule of its existing test (`test_kernels_gpu.py`,
`test_attention_gpu.py`: bit-exact for the packers, casts and the max-pool, their tolerances for the rest, unchanged); the large
run's first period holds the bits of that run; every output item holds the bits of its index modulo 7 (each kernel computes an
item from its own input item in a fixed order); outputs come from `guard.Guard.patch` under 0xFF with clean bands; the operands'
first and last period are unchanged.  Each case prints its batch and sizes (`pytest -s`)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import attention_cases as ac  # noqa: E402
import big_cases as bc  # noqa: E402
from frmap_amd import ops, synth  # noqa: E402

K = bc.K
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _tol(dtype):             # as test_kernels_gpu.py / test_attention_gpu.py
    return (2e-3, 2e-3) if dtype == torch.float16 else (1.6e-2, 1.6e-2)


def _randn(seed, shape, tag, dtype=torch.float32):
    return synth.randn(seed, (K,) + tuple(shape), tag).to(dtype)


def _nchw(t):
    return t.float().permute(0, 3, 1, 2)


def build(op):
    """(blocks, call, check_first) of a table entry."""
    dt, name = op.dtype, op.name
    shape = {n: s for n, (s, _) in op.inputs.items()}
    atol, rtol = _tol(dt)
    if name.startswith("pack_input"):
        x = _randn(901, shape["x"], "x")

        def check(o):
            assert torch.equal(o[0][..., :3], x.permute(0, 2, 3, 1).to(dt)) and float(o[0][..., 3].float().abs().max()) == 0.0
        return {"x": x}, lambda d: (ops.pack_input(d["x"], dt),), check
    if name == "normalize_u8":
        g = torch.Generator().manual_seed(902)
        img = torch.randint(0, 256, (K,) + shape["img"], generator=g).to(torch.uint8)
        ref = (img.permute(0, 3, 1, 2).float().div(255) - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)

        def check(o):
            assert torch.allclose(o[0], ref, atol=1e-6, rtol=1e-6)
            assert torch.equal(o[1][..., :3].float(), ref.permute(0, 2, 3, 1).to(dt).float()) and float(o[1][..., 3].float().abs().max()) == 0.0
        return {"img": img}, lambda d: ops.normalize_u8(d["img"], MEAN, STD, want_nchw=True, nhwc4_dtype=dt), check
    if name == "cast_to_f32":
        x = _randn(903, shape["x"], "c", dt)
        return {"x": x}, lambda d: (ops.cast_to_f32(d["x"]),), lambda o: _eq(o[0], x.float())
    if name == "cast_from_f32":
        x = _randn(904, shape["x"], "c")
        return {"x": x}, lambda d: (ops.cast_from_f32(d["x"], dt),), lambda o: _eq(o[0], x.to(dt))
    if name == "maxpool":
        x = _randn(905, shape["x"], "x", dt)
        return {"x": x}, lambda d: (ops.maxpool(d["x"], 3, 1, 1),), lambda o: _eq(_nchw(o[0]), F.max_pool2d(_nchw(x), 3, 1, 1))
    if name == "avgpool_global":
        x = _randn(906, shape["x"], "x", dt)
        return {"x": x}, lambda d: (ops.avgpool_global(d["x"]),), lambda o: _close(o[0], _nchw(x).mean(dim=(2, 3)), 1e-5, 1e-5)
    if name == "avgpool_adaptive":
        x = _randn(907, shape["x"], "x", dt)
        return {"x": x}, lambda d: (ops.avgpool_adaptive(d["x"], 2, 2),), lambda o: _close(_nchw(o[0]), F.adaptive_avg_pool2d(_nchw(x), (2, 2)), atol, rtol)
    if name.startswith("add_pos_layernorm"):
        L, D = shape["x"]
        x = _randn(908, (L, D), "x", dt)
        pos = synth.randn(909, (L, D), "p") * 0.1
        gamma, beta = synth.randn(910, (D,), "g").abs() + 0.5, synth.randn(911, (D,), "b") * 0.1
        t_ref, y_ref = ac.add_pos_layernorm_ref(x, pos, gamma, beta, True)
        dev = [t.to("cuda") for t in (pos, gamma, beta)]

        def check(o):
            assert torch.equal(o[0], t_ref)
            _close(o[1].double(), y_ref, atol * 2, rtol)
        return {"x": x}, lambda d: ops.add_pos_layernorm(d["x"], dev[0], dev[1], dev[2], want_sum=True), check
    if name == "mha_tokens":
        L, D3 = shape["qkv"]
        H = D3 // 3 // ac.DH
        qkv = ac.mha_inputs("peaked", 912, K, L, H, dt)
        ref = ac.mha_ref(qkv, H)

        def check(o):
            raw, rule = ac.mha_ratio(o[0], ref)
            assert rule <= 1.0, (raw, rule)
        return {"qkv": qkv}, lambda d: (ops.mha_tokens(d["qkv"], H),), check
    if name == "mean_layernorm":
        L, D = shape["t"]
        t = (_randn(913, (L, D), "t") + 0.25).to(dt)
        gamma, beta = synth.randn(914, (D,), "g").abs() + 0.5, synth.randn(915, (D,), "b") * 0.1
        dev = [v.to("cuda") for v in (gamma, beta)]
        return {"t": t}, lambda d: (ops.mean_layernorm(d["t"], dev[0], dev[1]),), lambda o: _close(o[0].double(), ac.mean_layernorm_ref(t, gamma, beta), 2e-4, 1e-4)
    if name == "cnn_attention":
        Hh, Ww, C = shape["x"]
        Cq = (shape["qkv"][2] - C) // 2
        qkv, x, g, sw, sb = ac.cnn_attention_inputs(916, K, Hh, Ww, C, Cq, 1, dt)
        ref = ac.cnn_attention_ref(qkv, x, Cq, g, sw, sb)
        A = ac.cnn_attention_margin(qkv, x, Cq, g, sw, sb, ref)
        dev = [v.to("cuda") for v in (g, sw, sb)]

        def check(o):
            fm, fp, worst = ac.cnn_attention_fail(o[0], o[1], ref, A)
            assert not bool(fm.any()) and not bool(fp.any()), worst
        return {"qkv": qkv, "x": x}, lambda d: ops.cnn_attention(d["qkv"], d["x"], dev[0], dev[1], dev[2], Cq, want_map=True, want_pool=True), check
    if name == "l2_normalize":
        x = _randn(917, shape["x"], "x")
        return {"x": x}, lambda d: (ops.l2_normalize(d["x"], 1e-12),), lambda o: _close(o[0], F.normalize(x, p=2, dim=1, eps=1e-12), 1e-6, 1e-5)
    if name == "pairwise_distance":
        a, b = _randn(918, shape["a"], "a"), _randn(919, shape["b"], "b")
        dref = F.pairwise_distance(a, b)
        thr = float(dref.sort().values[K // 2] + dref.sort().values[K // 2 - 1]) / 2        # between two of the block's distances

        def check(o):
            assert torch.allclose(o[0], dref, rtol=1e-6) and o[1].tolist() == (dref < thr).int().tolist() and 0 < int(o[1].sum()) < K
        return {"a": a, "b": b}, lambda d: ops.pairwise_distance(d["a"], d["b"], thr), check
    if name == "linear_f32":
        Kd = shape["x"][0]
        N = op.outputs[0][0][0]
        x, w = _randn(920, (Kd,), "x"), synth.randn(921, (N, Kd), "w") / Kd ** 0.5
        sc, sh = synth.randn(922, (N,), "s").abs() + 0.5, synth.randn(923, (N,), "h")
        ref = (x.double() @ w.double().t()) * sc.double() + sh.double()
        dev = [v.to("cuda") for v in (w, sc, sh)]
        return {"x": x}, lambda d: (ops.linear_f32(d["x"], dev[0], dev[1], dev[2], False),), lambda o: _close(o[0].double(), ref, 2e-5, 2e-5)
    raise ValueError(name)


def _eq(got, want):
    assert got.dtype == want.dtype and torch.equal(got, want)


def _close(got, want, atol, rtol):
    assert torch.allclose(got, want.to(got.dtype), atol=atol, rtol=rtol), float((got.double() - want.double()).abs().max())


@pytest.mark.parametrize("op", bc.BIG_LAYOUT, ids=[o.name for o in bc.BIG_LAYOUT])
def test_op_past_the_offset_marks(op):
    blocks, call, check = build(op)
    for n, (s, d) in op.inputs.items():
        assert tuple(blocks[n].shape) == (K,) + tuple(s) and blocks[n].dtype == d, (op.name, n)
    B = bc.op_batch(op)
    for what, value, bound in op.limits:
        assert value(B) < bound, (op.name, what, value(B), bound)

    def checked(outs):
        assert [(tuple(t.shape[1:]), t.dtype) for t in outs] == [(tuple(s), d) for s, d in op.outputs], op.name
        check(outs)
    got_B, sizes = bc.run_periodic(op.name, blocks, call, checked, [ops], B=B, small_outputs=op.small)
    assert got_B == B and sum(sizes.values()) == sum(B * o.item_bytes for o in bc.op_operands(op)[1])
