"""GPU: the token and attention kernels (`csrc/transformer.hip`) on every path they branch on, against the float64
references of `attention_cases.py` computed from the same rounded operands.

* `mha_tokens`: every count of padded key rows and of all-padding waves (L = 1 ... 64), H = 1, 2, 4, 8, on inputs where a wrong
  key mask, a transposed matrix or a wrong scale is an O(1) error; acceptance `|out - O| <= 2 u (P @ |V| + |O|) + 1e-6`.
* `cnn_attention`: all four template instances (CPT 1 / 2 x LMAX 49 / 64), non-square maps, KS = 1 and KS wider than the map,
  Cq = 8 and 128, map-only and pool-only output; acceptance `2 u |want| + A` with A from the reference's own fp32 error.
* `add_pos_layernorm`: the one- and two-block 16-byte paths and the scalar path; `mean_layernorm`: 2 and 4 token subsets,
  fewer tokens than a round, exactly one round, many rounds, and the scalar fallback.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from frmap_amd import _lib, ops, synth  # noqa: E402

import attention_cases as ac  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]


def _tol(dtype):
    # as test_kernels_gpu.py: one rounding of the output to the storage dtype + fp32 accumulation noise
    return (2e-3, 2e-3) if dtype == torch.float16 else (1.6e-2, 1.6e-2)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------------------------------------------------------------------------
# mha_tokens
# --------------------------------------------------------------------------------------------------------------------------------
def _check_mha(family, seed, B, L, H, dtype):
    qkv = ac.mha_inputs(family, seed, B, L, H, dtype)
    out = ops.mha_tokens(qkv.to(DEV), H).cpu()
    assert out.shape == (B, L, H * ac.DH) and out.dtype == dtype
    raw, rule = ac.mha_ratio(out, ac.mha_ref(qkv, H))
    print(f"mha_tokens B={B} L={L} H={H} {family} {str(dtype)[6:]}: worst err = {raw:.3f} u (P@|V| + |O|)")
    assert rule <= 1.0, (family, B, L, H, dtype, raw, rule)
    return raw


# L = 64: no key masked; 49 ... 63: padded keys inside the last wave's tile; 33 / 48: wave 3 all padding; 17 / 32: waves 2-3;
# 1 / 15 / 16: waves 1-3 (16: the last query tile exactly full); H = 1, 2, 4, 8: D = 128, 256, 512, 1024
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,H", [(1, 1), (15, 2), (16, 4), (17, 4), (32, 1), (33, 8), (48, 4), (49, 4), (63, 1), (64, 2), (64, 8)])
def test_mha_tokens_every_padding_and_head_count(L, H, dtype):
    """Peaked inputs (mean top probability ~ 0.6: a transposed P or a wrong scale is an O(1) error) and mask-sensitive inputs
    (real logits ~ -19: one admitted padded key takes all the weight) at every L where the number of padded keys, of padded
    query rows and of all-padding waves changes; (49, 4), the model's shape, also on the flat inputs the older test uses."""
    for fam in ("peaked", "mask_sensitive") + (("flat",) if (L, H) == (49, 4) else ()):
        _check_mha(fam, 500 + L + H, 3, L, H, dtype)


def test_mha_tokens_more_workgroups_than_compute_units():
    """B = 70, H = 4: 280 workgroups of 78 KB LDS, more than one round over the 256 CUs."""
    _check_mha("peaked", 571, 70, 17, 4, torch.float16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mha_tokens_batch_independent(dtype):
    """Face b of a B = 5 call is bit-identical to the same face alone (one workgroup per face and head, nothing shared)."""
    qkv = ac.mha_inputs("peaked", 580, 5, 33, 4, dtype).to(DEV)
    full = ops.mha_tokens(qkv, 4)
    for b in (0, 3, 4):
        assert torch.equal(ops.mha_tokens(qkv[b:b + 1].contiguous(), 4)[0], full[b]), b


def test_mha_tokens_refusals_launch_nothing():
    """L = 0, L = 65 and D != 128 H return -1 from the library and leave the output untouched; a float32 qkv never gets there."""
    lib = _lib.load()
    qkv = torch.zeros((2, 65, 3 * 256), dtype=torch.float16, device=DEV)
    out = torch.full((2, 65, 256), 7.0, dtype=torch.float16, device=DEV)
    for L, D, H in ((0, 256, 2), (65, 256, 2), (49, 256, 4), (49, 192, 2)):
        assert lib.frmap_mha_tokens(qkv.data_ptr(), out.data_ptr(), 2, L, D, H, ops.F16, _stream()) == -1, (L, D, H)
        assert b"mha_tokens" in lib.frmap_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for shape in ((2, 0, 768), (2, 65, 768)):
        with pytest.raises(ValueError):
            ops.mha_tokens(torch.zeros(shape, dtype=torch.float16, device=DEV), 2)
    with pytest.raises(ValueError):
        ops.mha_tokens(torch.zeros((2, 49, 768), dtype=torch.float16, device=DEV), 4)
    with pytest.raises(TypeError):
        ops.mha_tokens(torch.zeros((2, 49, 768), dtype=torch.float32, device=DEV), 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [17, 49])
def test_mha_tokens_writes_only_its_output(L, dtype):
    """Guard band: the output is a slice in the middle of a sentinel-filled buffer (rows >= L of the padded 64-row tile must
    not be stored, nor anything before row 0)."""
    B, H, G = 3, 2, 4096
    D = H * ac.DH
    qkv = ac.mha_inputs("peaked", 590 + L, B, L, H, dtype).to(DEV)
    buf = torch.full((2 * G + B * L * D,), 7.0, dtype=dtype, device=DEV)
    mid = buf[G:G + B * L * D]
    assert _lib.load().frmap_mha_tokens(qkv.data_ptr(), mid.data_ptr(), B, L, D, H, ops.dt_code(dtype), _stream()) == 0
    torch.cuda.synchronize()
    assert bool((buf[:G] == 7.0).all()) and bool((buf[G + B * L * D:] == 7.0).all())
    assert torch.equal(mid.view(B, L, D), ops.mha_tokens(qkv, H))


# --------------------------------------------------------------------------------------------------------------------------------
# cnn_attention
# --------------------------------------------------------------------------------------------------------------------------------
# H, W, C, Cq, KS, want_map, want_pool, refused        instance <CPT, LMAX>, what the case is for
CA_CASES = [
    (7, 7, 512, 64, 7, True, True, False),     # <2, 49> the model's shape
    (8, 8, 512, 64, 7, True, True, True),      # <2, 64> needs 183 808 B of LDS (> 160 KB): the documented refusal
    (8, 8, 512, 24, 7, True, True, False),     # <2, 64> with all 64 positions, the widest Cq that fits beside a 64 x 512 map
    (5, 11, 512, 8, 3, True, False, False),    # <2, 64> non-square, Cq at its minimum, map only
    (4, 9, 256, 32, 3, True, True, False),     # <1, 49> non-square (a gate convolution that swaps H and W fails 75 % here)
    (7, 9, 256, 128, 5, False, True, False),   # <1, 64> Cq at its maximum, pool only
    (1, 1, 256, 8, 1, True, True, False),      # <1, 49> one position: softmax of one logit, KS = 1
    (3, 3, 512, 24, 15, True, True, False),    # <2, 49> KS wider than the map: every tap of rows / columns 0..2 only
    (64, 1, 256, 32, 7, True, True, False),    # <1, 64> a column: the horizontal taps are all padding
    (1, 50, 512, 32, 3, True, True, False),    # <2, 64> a row, just above the 49-position instance
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W,C,Cq,KS,want_map,want_pool,refused", CA_CASES)
def test_cnn_attention_every_instance_and_border(H, W, C, Cq, KS, want_map, want_pool, refused, dtype):
    """Peaked inputs, gamma = 0.7 and gamma = 0 (then y = x exactly before the gate), a negative gate bias."""
    B = 3
    for gamma in (0.7, 0.0):
        qkv, x, g, sw, sb = ac.cnn_attention_inputs(600 + H * W + Cq, B, H, W, C, Cq, KS, dtype, gamma=gamma)
        args = (qkv.to(DEV), x.to(DEV), g.to(DEV), sw.to(DEV), sb.to(DEV), Cq)
        if refused:
            with pytest.raises(ValueError, match="LDS"):
                ops.cnn_attention(*args, want_map=want_map, want_pool=want_pool)
            continue
        om, op = ops.cnn_attention(*args, want_map=want_map, want_pool=want_pool)
        assert (om is None) == (not want_map) and (op is None) == (not want_pool)
        ref = ac.cnn_attention_ref(qkv, x, Cq, g, sw, sb)
        A = ac.cnn_attention_margin(qkv, x, Cq, g, sw, sb, ref)
        fm, fp, worst = ac.cnn_attention_fail(om.cpu() if want_map else None, op.cpu() if want_pool else None, ref, A)
        print(f"cnn_attention {H}x{W} C={C} Cq={Cq} KS={KS} gamma={gamma} {str(dtype)[6:]}: A = {A:.3g}, worst err / A = {worst:.3f}")
        assert fm is None or not bool(fm.any()), (gamma, int(fm.sum()), worst)
        assert fp is None or not bool(fp.any()), (gamma, int(fp.sum()), worst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cnn_attention_batch_independent_and_guarded(dtype):
    """Image b of a B = 5 call is bit-identical to the same image alone, and a map written into the middle of a sentinel-filled
    buffer leaves both sides untouched (L = 36 of the 49-position instance: positions 36..48 are never stored)."""
    B, H, W, C, Cq, KS = 5, 4, 9, 256, 32, 3
    qkv, x, g, sw, sb = (t.to(DEV) for t in ac.cnn_attention_inputs(650, B, H, W, C, Cq, KS, dtype))
    om, op = ops.cnn_attention(qkv, x, g, sw, sb, Cq, want_map=True, want_pool=True)
    for b in (0, 2, 4):
        m1, p1 = ops.cnn_attention(qkv[b:b + 1].contiguous(), x[b:b + 1].contiguous(), g, sw, sb, Cq, want_map=True, want_pool=True)
        assert torch.equal(m1[0], om[b]) and torch.equal(p1[0], op[b]), b
    G, n = 4096, B * H * W * C
    buf = torch.full((2 * G + n,), 7.0, dtype=dtype, device=DEV)
    pool = torch.full((G + B * C + G,), 7.0, dtype=torch.float32, device=DEV)
    rc = _lib.load().frmap_cnn_attention(qkv.data_ptr(), x.data_ptr(), g.data_ptr(), sw.data_ptr(), sb.data_ptr(),
                                         buf[G:].data_ptr(), pool[G:].data_ptr(), B, H, W, Cq, C, KS, ops.dt_code(dtype), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((buf[:G] == 7.0).all()) and bool((buf[G + n:] == 7.0).all())
    assert bool((pool[:G] == 7.0).all()) and bool((pool[G + B * C:] == 7.0).all())
    assert torch.equal(buf[G:G + n].view(B, H, W, C), om) and torch.equal(pool[G:G + B * C].view(B, C), op)


def test_cnn_attention_refusals():
    """H W = 65, C = 384, Cq = 12 and an even KS are refused, not run."""
    def call(H, W, C, Cq, KS):
        z = lambda *s: torch.zeros(s, dtype=torch.float16, device=DEV)
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
        return ops.cnn_attention(z(2, H, W, 2 * Cq + C), z(2, H, W, C), f(1), f(1, 2, KS, KS), f(1), Cq, want_map=True)
    for bad in ((5, 13, 256, 32, 3), (7, 7, 384, 32, 3), (7, 7, 256, 12, 3), (7, 7, 256, 32, 4)):
        with pytest.raises(ValueError, match="cnn_attention"):
            call(*bad)
    call(7, 7, 256, 32, 3)


# --------------------------------------------------------------------------------------------------------------------------------
# add_pos_layernorm
# --------------------------------------------------------------------------------------------------------------------------------
# D = 512: one 16-byte block per lane; 1024: two; 64, 192, 768, 960 (D % 512 != 0): the scalar path with 1, 3, 12, 15 elements
# per lane; 256: scalar, 9 rows.  Rows: 245, 21, 10, 147, 1, 6, 9 - multiples of the 4 rows of a workgroup and not.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,L,D", [(5, 49, 512), (3, 7, 1024), (2, 5, 64), (3, 49, 192), (1, 1, 768), (2, 3, 960), (9, 1, 256)])
def test_add_pos_layernorm_vector_and_scalar_paths(B, L, D, dtype):
    atol, rtol = _tol(dtype)
    x = synth.randn(700 + D, (B, L, D), "x").to(dtype)
    x[B - 1, L - 1, :] = 1.5                         # a constant row: variance 0, y = beta exactly, no NaN
    pos = synth.randn(701 + D, (L, D), "p") * 0.1
    gamma, beta = synth.randn(702, (D,), "g").abs() + 0.5, synth.randn(703, (D,), "b") * 0.1
    for p in (pos, None):
        for want_sum in (True, False):
            t, y = ops.add_pos_layernorm(x.to(DEV), None if p is None else p.to(DEV), gamma.to(DEV), beta.to(DEV), want_sum=want_sum)
            t_ref, y_ref = ac.add_pos_layernorm_ref(x, p, gamma, beta, want_sum)
            assert (t is None) == (not want_sum)
            if want_sum:
                assert torch.equal(t.cpu(), t_ref), (p is None, "t")
            y = y.cpu()
            assert torch.isfinite(y.float()).all()
            assert torch.allclose(y.double(), y_ref, atol=atol * 2, rtol=rtol), (p is None, want_sum, float((y.double() - y_ref).abs().max()))
            if p is None:
                assert torch.equal(y[B - 1, L - 1], beta.to(dtype)), "constant row"


def test_add_pos_layernorm_refusals():
    for D in (1088, 100):
        with pytest.raises(ValueError, match="add_pos_layernorm"):
            ops.add_pos_layernorm(torch.zeros((2, 3, D), dtype=torch.float16, device=DEV), None, torch.ones(D, device=DEV),
                                  torch.zeros(D, device=DEV))


# --------------------------------------------------------------------------------------------------------------------------------
# mean_layernorm
# --------------------------------------------------------------------------------------------------------------------------------
# 16-byte path (D % 8 == 0), a round = 7 loads x nsub token subsets:
#   D = 512 (nsub 4, round 28): L = 49 two rounds; 1 and 4 below one round (subsets with no token); 28 exactly one; 29 one token more
#   D = 1024, L = 64 and D = 768, L = 200: nsub 2 (round 14), 5 and 15 rounds, L > 49;  D = 64 / 8: 32 / 4 active threads
#   D = 1000: 125 groups x 2 subsets = 250 active threads, C / 8 does not divide 256
# scalar fallback (D % 8 != 0): D = 100 (one element per thread), D = 1001 (four)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,L,D", [(5, 49, 512), (3, 1, 512), (2, 4, 512), (2, 28, 512), (2, 29, 512), (2, 64, 1024), (3, 200, 768),
                                   (2, 10, 64), (2, 49, 8), (3, 13, 100), (2, 5, 1000), (2, 5, 1001)])
def test_mean_layernorm_subsets_rounds_and_fallback(B, L, D, dtype):
    t = (synth.randn(800 + D + L, (B, L, D), "t") + 0.25).to(dtype)
    gamma, beta = synth.randn(801, (D,), "g").abs() + 0.5, synth.randn(802, (D,), "b") * 0.1
    out = ops.mean_layernorm(t.to(DEV), gamma.to(DEV), beta.to(DEV)).cpu()
    ref = ac.mean_layernorm_ref(t, gamma, beta)
    assert torch.allclose(out.double(), ref, atol=2e-4, rtol=1e-4), float((out.double() - ref).abs().max())


def test_mean_layernorm_refusal():
    with pytest.raises(ValueError, match="mean_layernorm"):
        ops.mean_layernorm(torch.zeros((2, 3, 1032), dtype=torch.float16, device=DEV), torch.ones(1032, device=DEV),
                           torch.zeros(1032, device=DEV))
