"""Shared CPU code of the attention / token-kernel tests (`test_attention_cpu.py`, `test_attention_gpu.py`).

* float64 references of `mha_tokens`, `cnn_attention`, `add_pos_layernorm` and `mean_layernorm` that take the ALREADY ROUNDED
  fp16 / bf16 operands, so the only differences to a kernel are its own arithmetic and its final rounding;
* seeded input builders (`synth.randn`): `peaked` (logits of standard deviation ~ 4: a transposed attention matrix or a wrong
  scale moves the output by O(1)), `flat` (the `* 0.5` inputs of `test_transformer_token_kernels`: an almost uniform softmax)
  and `mask_sensitive` (every real logit near -19, so a padded zero key that is wrongly admitted takes nearly all the weight);
* the acceptance rules, as functions that return the observed fraction of the bound;
* fp32 emulations of the two attention kernels with switches that break them on purpose, so the CPU test can show that the
  acceptance rules reject a transposed matrix, a wrong scale, a key mask that is off by one and a gate convolution that swaps
  H and W.
"""
import math

import torch
import torch.nn.functional as F

from frmap_amd import synth

DH = 128                                   # head dim of mha_tokens
LP = 64                                    # mha_tokens pads the key axis to 64 zero rows
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # unit roundoff of the storage dtypes


# ------------------------------------------------------------------------------------------------------------------------------
# input builders
# ------------------------------------------------------------------------------------------------------------------------------
def mha_inputs(family, seed, B, L, H, dtype):
    """qkv [B, L, 3 * 128 H] in `dtype` (q | k | v, as nn.MultiheadAttention's in_proj emits them)."""
    D = H * DH
    r = synth.randn(seed, (B, L, 3 * D), "qkv." + family)
    q, k, v = r.split(D, dim=-1)
    if family == "peaked":                 # logit = q.k / sqrt(128): standard deviation 2 * 2 * sqrt(128) / sqrt(128) = 4
        q, k = q * 2.0, k * 2.0
    elif family == "flat":                 # standard deviation 0.25: an almost uniform softmax
        q, k, v = q * 0.5, k * 0.5, v * 0.5
    elif family == "mask_sensitive":       # logit ~ -128 * 1.3^2 / sqrt(128) = -19 for every real key, 0 for a padded zero key
        q, k = q.abs() + 0.5, -(k.abs() + 0.5)
    else:
        raise ValueError(family)
    return torch.cat([q, k, v], dim=-1).to(dtype)


def cnn_attention_inputs(seed, B, H, W, C, Cq, KS, dtype, gamma=0.7, bias=-0.3):
    """Peaked inputs of `cnn_attention`: (qkv [B,H,W,2Cq+C], x [B,H,W,C]) in `dtype`, gamma [1], spatial_w [1,2,KS,KS],
    spatial_b [1] in fp32.  q, k have standard deviation sqrt(32 / Cq) (1 at Cq = 32), v and x have 1."""
    s = math.sqrt(32.0 / Cq)
    q = synth.randn(seed, (B, H, W, Cq), "ca.q") * s
    k = synth.randn(seed, (B, H, W, Cq), "ca.k") * s
    v = synth.randn(seed, (B, H, W, C), "ca.v")
    x = synth.randn(seed, (B, H, W, C), "ca.x")
    sw = synth.randn(seed, (1, 2, KS, KS), "ca.sw") * (1.0 / KS)
    return (torch.cat([q, k, v], dim=-1).to(dtype), x.to(dtype), torch.tensor([gamma], dtype=torch.float32), sw,
            torch.tensor([bias], dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------------------------------------
def _heads(z, B, L, H):
    return z.reshape(B, L, H, DH).transpose(1, 2)             # [B, H, L, 128]


def mha_ref(qkv, H):
    """softmax(Q K^T / sqrt(128)) V per head in float64.  Returns (O [B,L,D], P [B,H,L,L], bound_terms [B,L,D]) with
    bound_terms = P @ |V| + |O|, the per-element magnitude the acceptance rule scales by the unit roundoff."""
    B, L, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (_heads(z, B, L, H) for z in qkv.double().split(D, dim=-1))
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(DH), dim=-1)
    O = (P @ v).transpose(1, 2).reshape(B, L, D)
    mag = (P @ v.abs()).transpose(1, 2).reshape(B, L, D)
    return O, P, mag + O.abs()


def cnn_attention_ref(qkv, x, Cq, gamma, sw, sb, dtype=torch.float64):
    """AttentionModule + SpatialAttention (`oracle/face_oracle.py:attention_module`) on an NHWC map and its packed q|k|v
    projection, plus the mean over positions, evaluated in `dtype` (float64: the reference; float32: its own rounding error).
    Returns (map [B,H,W,C], pool [B,C])."""
    B, H, W, C = x.shape
    L = H * W
    t = qkv.to(dtype).reshape(B, L, 2 * Cq + C)
    q, k, v = t[..., :Cq], t[..., Cq:2 * Cq], t[..., 2 * Cq:]
    attention = F.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)                    # [B, L(i), L(j)]
    out = torch.bmm(attention, v)                                                     # out[i][c] = sum_j attn[i][j] v[j][c]
    y = gamma.to(dtype) * out + x.to(dtype).reshape(B, L, C)
    pooled = torch.stack([y.mean(dim=2), y.max(dim=2)[0]], dim=1).reshape(B, 2, H, W)
    gate = torch.sigmoid(F.conv2d(pooled, sw.to(dtype).reshape(1, 2, sw.shape[-1], sw.shape[-1]), sb.to(dtype),
                                  padding=sw.shape[-1] // 2))
    m = y * gate.reshape(B, L, 1)
    return m.reshape(B, H, W, C), m.mean(dim=1)


def _layer_norm64(t, gamma, beta, eps):
    t = t.double()
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).mean(-1, keepdim=True)
    return (t - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def add_pos_layernorm_ref(x, pos, gamma, beta, want_sum, eps=1e-5):
    """(t, y): t = x (+ pos[l]), one fp32 add rounded to x's dtype (None unless `want_sum`); y = LayerNorm in float64 of the
    STORED t when it is stored (the residual stream lives in the storage dtype), of the fp32 sum otherwise."""
    t32 = x.float() + pos if pos is not None else x.float()
    t = t32.to(x.dtype) if want_sum else None
    return t, _layer_norm64(t if want_sum else t32, gamma, beta, eps)


def mean_layernorm_ref(t, gamma, beta, eps=1e-5):
    return _layer_norm64(t.double().mean(dim=1), gamma, beta, eps)


# ------------------------------------------------------------------------------------------------------------------------------
# acceptance rules
# ------------------------------------------------------------------------------------------------------------------------------
def mha_ratio(out, ref):
    """(worst err / (u * (P @ |V| + |O|)), worst err / (2 u (P @ |V| + |O|) + 1e-6)) of an `mha_tokens` output against
    `ref = mha_ref(...)`.  The second number is the acceptance rule: the output passes iff it is <= 1.

    Rounding P to the storage dtype moves the output by at most u * P @ |V|, rounding the output by at most u * |O|; the
    factor 2 is the margin over that worst case for fp32 accumulation order and `__expf`, both orders of magnitude below u."""
    O, _, terms = ref
    u = UNIT[out.dtype]
    err = (out.double() - O).abs()
    return float((err / (u * terms).clamp_min(1e-300)).max()), float((err / (2 * u * terms + 1e-6)).max())


def cnn_attention_margin(qkv, x, Cq, gamma, sw, sb, ref64):
    """A = max(16 * max|ref32 - ref64|, 2e-5): sixteen times the error the same formula makes in float32 on the CPU (the
    kernel also computes in fp32, in another order), floored at 2e-5.  Never derived from a kernel's output."""
    m32, p32 = cnn_attention_ref(qkv, x, Cq, gamma, sw, sb, dtype=torch.float32)
    e = max(float((m32.double() - ref64[0]).abs().max()), float((p32.double() - ref64[1]).abs().max()))
    return max(16.0 * e, 2e-5)


def cnn_attention_fail(got_map, got_pool, ref64, A):
    """Per-element failures of the rule `|map - want| <= 2 u |want| + A` (the stored map is rounded once) and `|pool - want|
    <= A` (fp32).  Returns (failing map mask | None, failing pool mask | None, worst err / A over what was given)."""
    worst, fm, fp = 0.0, None, None
    if got_map is not None:
        err = (got_map.double() - ref64[0]).abs()
        fm = err > 2 * UNIT[got_map.dtype] * ref64[0].abs() + A
        worst = max(worst, float(((err - 2 * UNIT[got_map.dtype] * ref64[0].abs()).clamp_min(0) / A).max()))
    if got_pool is not None:
        err = (got_pool.double() - ref64[1]).abs()
        fp = err > A
        worst = max(worst, float((err / A).max()))
    return fm, fp, worst


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' arithmetic, with switches that break them
# ------------------------------------------------------------------------------------------------------------------------------
def emulate_mha(qkv, H, dtype, *, mask_upto=None, transpose=False, scale=None):
    """`mha_tokens_kernel` in fp32 on the CPU: L padded to 64 zero rows, keys >= `mask_upto` (default L; 64 = no mask) get
    -inf, P rounded to `dtype` before P V, the output rounded to `dtype`.  `transpose` uses P^T, `scale` replaces 1/sqrt(128)."""
    B, L, D3 = qkv.shape
    D = D3 // 3
    pad = torch.zeros((B, LP, D3), dtype=torch.float32)
    pad[:, :L] = qkv.float()
    q, k, v = (_heads(z, B, LP, H) for z in pad.split(D, dim=-1))
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(DH) if scale is None else scale)
    keep = torch.arange(LP) < (L if mask_upto is None else mask_upto)
    s = torch.where(keep, s, torch.tensor(-math.inf))
    p = torch.softmax(s, dim=-1)
    if transpose:
        p = p.transpose(-1, -2)
    p = p.to(dtype).float()
    return (p @ v).transpose(1, 2).reshape(B, LP, D)[:, :L].to(dtype)


def emulate_cnn_attention(qkv, x, Cq, gamma, sw, sb, dtype, *, transpose=False, swap_hw=False):
    """`cnn_attention_kernel` in fp32 on the CPU; only the stored map is rounded.  `transpose` applies attn^T; `swap_hw` runs
    the gate convolution as if the L positions were a W x H image (`iy * H + ix`, `oy = i / H`).  Returns (map, pool)."""
    B, H, W, C = x.shape
    L, KS = H * W, sw.shape[-1]
    t = qkv.float().reshape(B, L, 2 * Cq + C)
    q, k, v = t[..., :Cq], t[..., Cq:2 * Cq], t[..., 2 * Cq:]
    a = F.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    if transpose:
        a = a.transpose(1, 2)
    y = gamma.float() * torch.bmm(a, v) + x.float().reshape(B, L, C)
    hh, ww = (W, H) if swap_hw else (H, W)
    pooled = torch.stack([y.mean(dim=2), y.max(dim=2)[0]], dim=1).reshape(B, 2, hh, ww)
    gate = torch.sigmoid(F.conv2d(pooled, sw.float().reshape(1, 2, KS, KS), sb.float(), padding=KS // 2))
    m = y * gate.reshape(B, L, 1)
    return m.reshape(B, H, W, C).to(dtype), m.mean(dim=1)
