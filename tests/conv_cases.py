"""Shared CPU code of the conv-family tests (`test_conv_cpu.py`, `test_conv_exact_gpu.py`, `test_conv_bound_gpu.py`).

Two instruments, neither with a tuned tolerance:

* EXACT INTEGERS.  Inputs and weights in {-1, 0, 1}, shift and residual integers in [-8, 8], so that S (the same op on the
  absolute values) is <= 256 for every output.  Every partial sum, in any order, chunking or split-K merge, is then an integer
  of magnitude <= 256: exact in fp32, fp16 and bf16.  The kernel must reproduce the float64 reference bit for bit; a dropped
  (tap, cin) product, a wrong padding or a wrong pixel / channel index moves an output by >= 1.
* ONE ROUNDING.  `|y - act(ref)| <= u |act(ref)| + C_ACC 2^-24 S` with u the unit roundoff of the storage dtype: the single
  final rounding `conv_epilogue` documents, plus an allowance for fp32 accumulation that is measured on CPU restatements
  (`test_conv_cpu.py`), never on a kernel.

Contents: float64 references (tap loops and explicit window maxima: independent of `F.conv2d` / `F.max_pool2d` / `F.gelu`,
which the CPU test compares them with), operand builders (exact integers, Gaussian, post-ReLU, the fp16 pair x 2^12 / w 2^-12
whose weights are subnormal), an fp32 emulation of the kernels' arithmetic with switches that break it on purpose, the case
tables of the two GPU files and the code that runs a case through the C ABI.  Every conv-family case names the kernel
instantiation it is about (`key`); `launch_case` asserts it before the launch and `test_conv_census_cpu.py` holds that the tables
together reach every instantiation there is.
"""
import math
import zlib
from collections import namedtuple

import torch

from frmap_amd import synth

UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # unit roundoff of the storage dtypes
EPS32 = 2.0 ** -24                                                # unit roundoff of the fp32 accumulator
C_ACC = 8.0                # fp32 accumulation allowance, in units of 2^-24 S (4 x the CPU restatements' worst, as a power of two)
GELU_LIP = 1.13            # max |gelu'(v)| (1.1289 at v = 1.41): how far GELU can stretch a pre-activation error
S_MAX_EXACT = 256.0
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
CHUNK = 32                 # input channels per k-step of every MFMA conv kernel


# ------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------------------------------------
def _pad(x, pad, replicate=False):
    if pad == 0:
        return x
    B, C, H, W = x.shape
    if replicate:
        iy = torch.arange(-pad, H + pad).clamp(0, H - 1)
        ix = torch.arange(-pad, W + pad).clamp(0, W - 1)
        return x[:, :, iy][:, :, :, ix]
    xp = x.new_zeros((B, C, H + 2 * pad, W + 2 * pad))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    return xp


def _tap(xp, w, ky, kx, stride, Ho, Wo):
    """One kernel tap: sum_c xp[b, c, oy s + ky, ox s + kx] w[o, c, ky, kx], in the operands' dtype."""
    xs = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
    return torch.einsum("bchw,oc->bohw", xs, w[:, :, ky, kx])


def conv_sum(x, w, stride, pad):
    """sum over taps and channels (no shift), NCHW, in the dtype of `x` / `w`."""
    k = w.shape[-1]
    Ho, Wo = (x.shape[2] + 2 * pad - k) // stride + 1, (x.shape[3] + 2 * pad - k) // stride + 1
    xp = _pad(x, pad)
    out = x.new_zeros((x.shape[0], w.shape[0], Ho, Wo))
    for ky in range(k):
        for kx in range(k):
            out += _tap(xp, w, ky, kx, stride, Ho, Wo)
    return out


def conv_ref(x, w, shift, stride=1, pad=None, residual=None):
    """conv k x k (stride, pad; default pad k // 2) + shift (+ residual) of the ALREADY ROUNDED operands, float64, NCHW, before the
    activation.  Returns (ref, S): S = the same op on |x|, |w|, |shift|, |residual|."""
    pad = w.shape[-1] // 2 if pad is None else pad
    x, w, sh = x.double(), w.double(), shift.double().view(1, -1, 1, 1)
    ref = conv_sum(x, w, stride, pad) + sh
    S = conv_sum(x.abs(), w.abs(), stride, pad) + sh.abs()
    if residual is not None:
        ref, S = ref + residual.double(), S + residual.double().abs()
    return ref, S


def conv_shortcut_ref(h, w, shift, xd, wd, ds_stride):
    """conv3x3 s1 p1 (h) + conv1x1 stride s (xd) + shift: BasicBlock.conv2 with its projection shortcut folded in."""
    ref, S = conv_ref(h, w, shift)
    xd, wd = xd.double(), wd.double()
    return ref + conv_sum(xd, wd, ds_stride, 0), S + conv_sum(xd.abs(), wd.abs(), ds_stride, 0)


def conv_pool2_ref(x, w, shift):
    """conv3x3 s1 p1 + shift BEFORE the fused MaxPool2d(2, 2): pool with `pooled(ref, S, act, 2, 2, 0)`."""
    return conv_ref(x, w, shift)


def small_cin_ref(x, w, shift, stride, pad):
    """The Cin = 3 first layers: 7x7 stride 2 pad 3 and 3x3 stride 1 pad 1."""
    return conv_ref(x, w, shift, stride, pad)


def stem_ref(x, w, shift):
    """conv 7x7 s2 p3 + shift BEFORE the fused pool: `pooled(ref, S, ACT_RELU, 3, 2, 1)` (ResNet) or `(..., 2, 2, 0)` (Siamese)."""
    return conv_ref(x, w, shift, 2, 3)


def linear_ref(x, w, shift, residual=None):
    """x [M, K] . w [N, K]^T + shift (+ residual), float64.  Returns (ref, S) as [M, N]."""
    x, w, sh = x.double(), w.double(), shift.double()
    ref, S = x @ w.t() + sh, x.abs() @ w.abs().t() + sh.abs()
    if residual is not None:
        ref, S = ref + residual.double(), S + residual.double().abs()
    return ref, S


def act64(v, act):
    """The activation in float64; GELU is the erf form `conv_epilogue` documents (nn.GELU's default)."""
    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))
    return v


def window_max(t, k, stride, pad):
    """max over k x k windows (stride, -inf padding, floor mode) of a float64 NCHW map, by explicit strided slices."""
    B, C, H, W = t.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    tp = t.new_full((B, C, H + 2 * pad, W + 2 * pad), -math.inf)
    tp[:, :, pad:pad + H, pad:pad + W] = t
    out = t.new_full((B, C, Ho, Wo), -math.inf)
    for dy in range(k):
        for dx in range(k):
            out = torch.maximum(out, tp[:, :, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride])
    return out


def pooled(ref, S, act, k, stride, pad):
    """(window max of act(ref) in float64, window max of S): what a fused conv + max-pool must store, and the magnitude its
    accumulation allowance scales with (|max a_i - max b_i| <= max |a_i - b_i|; the maximum is rounded once)."""
    return window_max(act64(ref, act), k, stride, pad), window_max(S, k, stride, pad)


# ------------------------------------------------------------------------------------------------------------------------------
# acceptance rules
# ------------------------------------------------------------------------------------------------------------------------------
def one_rounding_ratio(y, want, S, dtype, lip=1.0):
    """max of |y - want| / (u |want| + lip C_ACC 2^-24 S): the output passes iff this is <= 1."""
    bound = UNIT[dtype] * want.abs() + lip * C_ACC * EPS32 * S
    return float(((y.double() - want).abs() / bound).max())


def assert_sharp(want, S, dtype, what=""):
    """The sharpness condition of `assert_one_rounding`, on the float64 reference alone (no kernel): the accumulation allowance at
    the largest S is at most a quarter of the rounding term at the mean output.  Returns the ratio of the two."""
    slack = C_ACC * EPS32 * float(S.max()) / (UNIT[dtype] * float(want.abs().mean()) / 4)
    assert slack <= 1.0, (what, "case drowns the rounding term: c 2^-24 max S = %.3f x (u mean|ref| / 4)" % slack)
    return slack


def assert_one_rounding(y, ref, S, dtype, act=ACT_NONE, what=""):
    """`|y - act(ref)| <= u |act(ref)| + c 2^-24 S` (GELU: the second term times 1.13) on every element; `ref` is the float64
    pre-activation (for a pooled op: the pooled activation, with act = ACT_NONE).  Also asserts that the case keeps the rule
    sharp: the accumulation allowance at the largest S is at most a quarter of the rounding term at the mean output.
    Returns the worst observed fraction of the bound."""
    want = act64(ref, act)
    assert tuple(y.shape) == tuple(want.shape), (what, tuple(y.shape), tuple(want.shape))
    u = UNIT[dtype]
    assert_sharp(want, S, dtype, what)
    ratio = one_rounding_ratio(y, want, S, dtype, GELU_LIP if act == ACT_GELU else 1.0)
    if not ratio <= 1.0:
        err = (y.double() - want).abs() / (u * want.abs() + (GELU_LIP if act == ACT_GELU else 1.0) * C_ACC * EPS32 * S)
        idx = [int(i) for i in torch.nonzero(err == err.max())[0]]
        raise AssertionError(f"{what}: |y - ref| reaches {ratio:.2f} x (u |ref| + {C_ACC:g} 2^-24 S) at {idx}: "
                             f"y = {float(y.double()[tuple(idx)])!r}, ref = {float(want[tuple(idx)])!r}, S = {float(S[tuple(idx)]):.4g}; "
                             f"{int((err > 1).sum())} of {err.numel()} outputs over the bound")
    return ratio


def assert_exact(y, ref, act=ACT_NONE, what=""):
    """The stored values equal float64 `act(ref)`; on a mismatch the message names the failing (image, channel, y, x) pattern."""
    want = act64(ref, act)
    assert act != ACT_GELU, "GELU is not exact"
    assert tuple(y.shape) == tuple(want.shape), (what, tuple(y.shape), tuple(want.shape))
    got = y.double()
    if torch.equal(got, want):
        return
    bad = torch.nonzero(got != want)
    dims = ["%s in %s" % (n, sorted(set(bad[:, d].tolist()))[:12]) for d, n in enumerate("nchw" if bad.shape[1] == 4 else "mn")]
    i = tuple(int(v) for v in bad[0])
    raise AssertionError(f"{what}: {bad.shape[0]} of {want.numel()} outputs differ from the exact integers ({'; '.join(dims)}); "
                         f"first at {i}: got {float(got[i])}, want {float(want[i])}")


# ------------------------------------------------------------------------------------------------------------------------------
# operand builders.  Every builder returns a dict of CPU tensors: x [B,Cin,H,W], w [Cout,Cin,k,k], shift [Cout] (fp32),
# r (residual, output-shaped, or None) and, with a shortcut, xd [B,dsC,Hd,Wd], wd [Cout,dsC,1,1].  x, w, r, xd, wd hold values
# the storage dtype represents exactly.
# ------------------------------------------------------------------------------------------------------------------------------
def _out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _coprime_stride(P):
    for q in (37, 41, 43, 47, 53, 59, 61, 67):
        if math.gcd(q, P) == 1:
            return q
    raise ValueError(P)


def exact_weights(seed, Cout, Cin, k, n_nz):
    """[Cout, Cin, k, k] float64 in {-1, 0, 1} with min(n_nz, k k Cin) nonzeros per output channel.  Positions are numbered
    p = (ky k + kx) Cin + c; channel o takes the n_nz positions ((o n_nz + i) q) mod P, q coprime to P: the runs of consecutive
    channels tile the position ring (every position is hit floor(Cout n_nz / P) times or once more) and one channel's set is
    spread q apart, across every tap and 32-channel chunk, not one contiguous run."""
    g = torch.Generator().manual_seed(seed)
    P = k * k * Cin
    n = min(n_nz, P)
    q = _coprime_stride(P)
    pos = ((torch.arange(Cout).view(-1, 1) * n + torch.arange(n).view(1, -1)) * q) % P
    w = torch.zeros((Cout, P), dtype=torch.float64)
    w.scatter_(1, pos, torch.randint(0, 2, (Cout, n), generator=g).double() * 2 - 1)
    return w.view(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()


def exact_operands(seed, B, H, W, Cin, Cout, k, stride=1, pad=None, res=False, n_nz=200, ds=None):
    """Exact-integer operands (float64).  ds = (dsC, ds_stride) adds the shortcut's xd, wd; callers then pass an n_nz that leaves
    room for both sums (n_nz main + min(n_nz, dsC) shortcut + 8 <= 256)."""
    g = torch.Generator().manual_seed(seed + 1)
    pad = k // 2 if pad is None else pad
    Ho, Wo = _out_hw(H, W, k, stride, pad)
    o = {"x": torch.randint(-1, 2, (B, Cin, H, W), generator=g).double(), "w": exact_weights(seed, Cout, Cin, k, n_nz),
         "shift": torch.randint(-8, 9, (Cout,), generator=g).float(), "r": None}
    if res:
        o["r"] = torch.randint(-8, 9, (B, Cout, Ho, Wo), generator=g).double()
    if ds is not None:
        dsC, sd = ds
        o["xd"] = torch.randint(-1, 2, (B, dsC, (H - 1) * sd + 1 + (sd - 1), (W - 1) * sd + 1 + (sd - 1)), generator=g).double()
        o["wd"] = exact_weights(seed + 2, Cout, dsC, 1, n_nz)
    return o


def coverage_min(w):
    """fewest output channels in which a (tap, cin) position of `w` is nonzero."""
    return int((w != 0).sum(dim=0).min())


def assert_exact_conditions(o, S, what=""):
    """(a) S <= 256 on every output: every partial sum is an integer all three formats hold exactly; (b) every (tap, cin)
    position, of the main weights and of the shortcut's, is nonzero in at least two output channels: no product can go missing
    unseen.  Also: the values are the integers the construction promises."""
    assert float(S.max()) <= S_MAX_EXACT, (what, "S max", float(S.max()))
    for key in ("w", "wd"):
        if o.get(key) is not None:
            assert coverage_min(o[key]) >= 2, (what, key, "a (tap, cin) position is covered", coverage_min(o[key]), "times")
            assert set(o[key].unique().tolist()) <= {-1.0, 0.0, 1.0}, (what, key)
    for key in ("x", "xd"):
        if o.get(key) is not None:
            assert set(o[key].unique().tolist()) <= {-1.0, 0.0, 1.0}, (what, key)
    for key in ("shift", "r"):
        if o.get(key) is not None:
            t = o[key].double()
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 8, (what, key)


def float_operands(family, seed, B, H, W, Cin, Cout, k, dtype, stride=1, pad=None, res=False, ds=None, w_gain=None, shift_std=0.1):
    """Seeded floating operands rounded to `dtype`.  family: 'gauss' (N(0,1) inputs, as the older tests), 'relu' (max(N(0,1), 0):
    non-negative with a non-zero mean, what a layer behind a ReLU really sees) or 'subnormal' (fp16 only: x 2^12 and w 2^-12, the
    same products with most weights in fp16's subnormal range).  Weights are N(0, w_gain / fan_in), w_gain 2 for 3x3 / 7x7, 1
    for 1x1, as in `test_kernels_gpu.py`."""
    pad = k // 2 if pad is None else pad
    Ho, Wo = _out_hw(H, W, k, stride, pad)
    gain = (2.0 if k > 1 else 1.0) if w_gain is None else w_gain
    x = synth.randn(seed, (B, Cin, H, W), "cc.x")
    w = synth.randn(seed, (Cout, Cin, k, k), "cc.w") * math.sqrt(gain / (Cin * k * k))
    if family == "relu":
        x = x.relu()
    elif family == "subnormal":
        assert dtype == torch.float16
        x, w = x * 4096.0, w / 4096.0
    elif family != "gauss":
        raise ValueError(family)
    o = {"x": x.to(dtype), "w": w.to(dtype), "shift": synth.randn(seed, (Cout,), "cc.b") * shift_std, "r": None}
    if family == "subnormal":
        sub = (o["w"].float().abs() < 2.0 ** -14) & (o["w"] != 0)
        assert float(sub.float().mean()) > 0.5, "the scaled weights were meant to be subnormal"
    if res:
        o["r"] = synth.randn(seed, (B, Cout, Ho, Wo), "cc.r").to(dtype)
    if ds is not None:
        dsC, sd = ds
        xd = synth.randn(seed, (B, dsC, (H - 1) * sd + 1 + (sd - 1), (W - 1) * sd + 1 + (sd - 1)), "cc.xd")
        wd = synth.randn(seed, (Cout, dsC, 1, 1), "cc.wd") * math.sqrt(1.0 / dsC)
        if family == "relu":
            xd = xd.relu()
        elif family == "subnormal":
            xd, wd = xd * 4096.0, wd / 4096.0
        o["xd"], o["wd"] = xd.to(dtype), wd.to(dtype)
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' arithmetic, with switches that break it
# ------------------------------------------------------------------------------------------------------------------------------
def emulate_conv(o, dtype, stride=1, pad=None, act=ACT_NONE, *, chunk_round=False, splitk_storage=False, round_before_residual=False,
                 tanh_gelu=False, drop_term=None, replicate_pad=False, shift_storage=False, want_fp32=False):
    """The conv of operand dict `o` as the kernels compute it: an fp32 accumulator that takes one 32-channel chunk of one tap at
    a time, then + shift (+ residual) in fp32, the activation in fp32, ONE rounding to `dtype`.  Returns the stored NCHW tensor
    (`want_fp32`: the fp32 value before that rounding, pre-activation).  Switches, each a defect the acceptance rules must reject:

    chunk_round            the accumulator is rounded to `dtype` after every 32-channel chunk
    splitk_storage         two split-K halves, the first merged through `dtype` (a wrong LDS merge of the KS = 2 layouts)
    round_before_residual  the conv + shift is rounded before the residual is added: two roundings
    tanh_gelu              tanh-GELU in place of erf-GELU
    drop_term=(o, c, ky, kx)  one (tap, cin) product of one output channel is left out
    replicate_pad          border pixels replicated in place of zero padding
    shift_storage          shift rounded to `dtype` (NOT caught by the bound at fp16, Cin 512: listed in DESIGN.md)"""
    x, w = o["x"].float(), o["w"].float().clone()
    k = w.shape[-1]
    pad = k // 2 if pad is None else pad
    Cin = x.shape[1]
    Ho, Wo = _out_hw(x.shape[2], x.shape[3], k, stride, pad)
    if drop_term is not None:
        w[drop_term] = 0.0
    xp = _pad(x, pad, replicate_pad)
    nch = (Cin + CHUNK - 1) // CHUNK

    def accumulate(chunks):
        acc = torch.zeros((x.shape[0], w.shape[0], Ho, Wo), dtype=torch.float32)
        for ci in chunks:
            c0, c1 = ci * CHUNK, min(Cin, (ci + 1) * CHUNK)
            for ky in range(k):
                for kx in range(k):
                    acc = acc + _tap(xp[:, c0:c1], w[:, c0:c1], ky, kx, stride, Ho, Wo)
            if chunk_round:
                acc = acc.to(dtype).float()
        return acc

    if splitk_storage:
        acc = accumulate(range(0, nch // 2)).to(dtype).float() + accumulate(range(nch // 2, nch))
    else:
        acc = accumulate(range(nch))
    sh = o["shift"].float()
    if shift_storage:
        sh = sh.to(dtype).float()
    v = acc + sh.view(1, -1, 1, 1)
    if o.get("r") is not None:
        if round_before_residual:
            v = v.to(dtype).float()
        v = v + o["r"].float()
    if want_fp32:
        return v
    if act == ACT_RELU:
        v = v.clamp_min(0)
    elif act == ACT_GELU:
        v = torch.nn.functional.gelu(v, approximate="tanh") if tanh_gelu else 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))
    return v.to(dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# case tables of the GPU files: the smallest entries of the tables in `test_kernels_gpu.py` for every kernel variant they force
# ------------------------------------------------------------------------------------------------------------------------------
# key: the kernel instantiation the case is about (`ops.conv_plan_key`, asserted just before the launch; None: no conv plan - the
# Cin = 3 and stem kernels).  im / pitch / wstart: frmap_conv_pp_im / frmap_conv_pp_pitch / frmap_conv_wave_start (None: not set).
Case = namedtuple("Case", "name file op B H W Cin Cout k stride res act tune ri ds query key im pitch wstart", defaults=(None,) * 4)
PP_OFF = (0, -1, -1)       # frmap_conv_pp_tuning arguments: first-generation kernels only


def _c(name, file, op, B, H, W, Cin, Cout, k=3, stride=1, res=False, act=ACT_RELU, tune=None, ri=None, ds=None, query=None,
       key=None, im=None, pitch=None, wstart=None):
    return Case(name, file, op, B, H, W, Cin, Cout, k, stride, res, act, tune, ri, ds, query, key, im, pitch, wstart)


IG, PP, SC, ST, S2D = "conv_igemm.hip", "conv_pp.hip", "conv_small_cin.hip", "stem_pool.hip", "stem_s2d.hip"

# query: (name of the layout / form query, the answers that assert the intended path).  The first-generation kernels have no
# query of their own: with the second generation switched off the layer's query must answer 0.
CONV_CASES = [
    # ---- conv_igemm.hip (frmap_conv_pp_tuning(0, -1, -1)) ----
    # (by the dispatcher's arithmetic the 10x6 and 7x7 maps, listed as "generic" in test_kernels_gpu.py, fit the register-prefetch
    #  kernel's 10 halo pieces per thread; the generic kernel takes halos past that: the 112-pixel-wide map)
    _c("wave-1patch", IG, "conv", 1, 8, 8, 64, 64, act=ACT_NONE, tune=PP_OFF, query=("conv3x3_pp", (0,)), key="conv3x3_c64_wave_kernel<2,EARLY>"),
    _c("wave-2tiles", IG, "conv", 3, 16, 24, 64, 128, res=True, tune=PP_OFF, query=("conv3x3_pp", (0,)), key="conv3x3_c64_wave_kernel<2,EARLY>"),
    _c("regprefetch", IG, "conv", 2, 20, 56, 64, 64, res=True, tune=PP_OFF, query=("conv3x3_pp", (0,)), key="conv3x3_fast_kernel<>"),
    _c("g1-odd-10x6", IG, "conv", 2, 10, 6, 32, 64, act=ACT_NONE, tune=PP_OFF, query=("conv3x3_pp", (0,)), key="conv3x3_fast_kernel<>"),
    _c("g1-c512-7x7", IG, "conv", 9, 7, 7, 512, 512, res=True, tune=PP_OFF, query=("conv3x3_pp", (0,)), key="conv3x3_fast_kernel<>"),
    _c("generic-112x112", IG, "conv", 1, 112, 112, 32, 64, tune=PP_OFF, query=("conv3x3_pp", (0,)), key="conv_igemm_kernel<256,3,1>"),   # halo past the register-prefetch limit
    _c("s2-split", IG, "conv", 4, 8, 6, 32, 128, stride=2, tune=PP_OFF, query=("conv3x3s2_pp", (0,)), key="conv3x3s2_split_kernel<>"),
    _c("s2-split-c256", IG, "conv", 2, 14, 14, 256, 512, stride=2, res=True, tune=PP_OFF, query=("conv3x3s2_pp", (0,)), key="conv3x3s2_fast_kernel<>"),
    _c("s2-oddH", IG, "conv", 3, 7, 10, 64, 128, stride=2, res=True, tune=PP_OFF, query=("conv3x3s2_pp", (0,)), key="conv_igemm_kernel<256,3,2>"),
    _c("1x1-gather-c64", IG, "conv", 2, 56, 56, 64, 128, k=1, stride=2, act=ACT_NONE, tune=PP_OFF, query=("conv1x1_pp", (0,)), key="conv_igemm_kernel<256,1,1>"),
    _c("1x1-gather-c128", IG, "conv", 2, 28, 28, 128, 256, k=1, stride=2, act=ACT_NONE, tune=PP_OFF, query=("conv1x1_pp", (0,)), key="conv1x1_kernel<4>"),
    _c("1x1-stage1", IG, "conv", 4, 13, 9, 160, 640, k=1, tune=PP_OFF, query=("conv1x1_pp", (0,)), key="conv1x1_kernel<1>"),
    # one k-step.  `frmap_conv_igemm` sends Cin < 128 to the first-generation 1x1 kernel whatever the tuning hook says (the
    # `Cin >= 128` test sits in front of `frmap_conv1x1_pp`), so the single-k-step path of `conv1x1_pp_kernel` cannot be reached
    # through the C ABI: `frmap_conv1x1_pp_layout` answers 2 for this shape under `frmap_conv_pp_tuning(1, -1, 256)`, but the kernel
    # that runs is this one.  No path assertion is made that the library cannot keep.
    _c("1x1-c32-1kstep", IG, "conv", 300, 1, 1, 32, 128, k=1, tune=PP_OFF, query=("conv1x1_pp", (0,)), key="conv_igemm_kernel<256,1,1>"),
    _c("linear-as-1x1", IG, "conv", 37, 1, 1, 1024, 512, k=1, tune=PP_OFF, query=("conv1x1_pp", (0,)), key="conv1x1_kernel<4>"),
    _c("g1-shortcut-3x5", IG, "ds", 1, 3, 5, 256, 128, ds=(256, 2), tune=PP_OFF, query=("conv3x3_pp_ds", (0,)), key="conv3x3_fast_kernel<DS>"),
    _c("g1-shortcut-10x6", IG, "ds", 4, 10, 6, 64, 128, ds=(32, 2), act=ACT_NONE, tune=PP_OFF, query=("conv3x3_pp_ds", (0,)), key="conv3x3_fast_kernel<DS>"),
    # ---- conv_pp.hip, 3x3 stride 1 ----
    _c("pp-bn128-ri0", PP, "conv", 5, 14, 14, 256, 256, res=True, tune=(1, -1, 128), ri=0, query=("conv3x3_pp", (2,)), key="conv3x3_pp_kernel<7,4,5,1>"),
    _c("pp-bn128-ri1", PP, "conv", 5, 14, 14, 256, 256, res=True, tune=(1, -1, 128), ri=1, query=("conv3x3_pp", (2,)), key="conv3x3_pp_kernel<7,4,5,1,RI>"),
    _c("pp-bn256-ri0", PP, "conv", 5, 14, 14, 256, 256, res=True, tune=(1, -1, 256), ri=0, query=("conv3x3_pp", (1,)), key="conv3x3_pp_kernel<7,2,3,1>"),
    _c("pp-bn256-ri1", PP, "conv", 5, 14, 14, 256, 256, res=True, tune=(1, -1, 256), ri=1, query=("conv3x3_pp", (1,)), key="conv3x3_pp_kernel<7,2,3,1,RI>"),
    _c("pp-splitk-ri0", PP, "conv", 2, 20, 12, 64, 128, tune=(1, -1, 1282), ri=0, query=("conv3x3_pp", (3,)), key="conv3x3_pp_kernel<7,2,6,2>"),
    # asks for interleaved reads and does NOT get them: with six halo pieces that form would spill (plan_pp_3x3), the planner
    # declines and the key is pp-splitk-ri0's.  The case holds the decline; split-K with the request honoured is cx-splitk4-ri1.
    _c("pp-splitk-ri1", PP, "conv", 2, 20, 12, 64, 128, tune=(1, -1, 1282), ri=1, query=("conv3x3_pp", (3,)), key="conv3x3_pp_kernel<7,2,6,2>"),
    _c("pp-splitk-res", PP, "conv", 3, 13, 17, 128, 256, res=True, act=ACT_NONE, tune=(1, -1, 1282), ri=0, query=("conv3x3_pp", (3,)), key="conv3x3_pp_kernel<7,2,6,2>"),
    _c("pp-px37-bn256", PP, "conv", 33, 7, 7, 128, 256, res=True, tune=(1, 37, 256), ri=0, query=("conv3x3_pp", (1,)), key="conv3x3_pp_kernel<7,2,3,1>"),
    _c("pp-px37-splitk", PP, "conv", 33, 7, 7, 128, 256, res=True, tune=(1, 37, 1282), ri=1, query=("conv3x3_pp", (3,)), key="conv3x3_pp_kernel<7,2,4,2,RI>"),
    _c("pp-1chunk", PP, "conv", 7, 5, 3, 32, 128, res=True, act=ACT_NONE, tune=(1, -1, -1), ri=0, query=("conv3x3_pp", (2,)), key="conv3x3_pp_kernel<7,4,3,1>"),
    # ---- conv_pp.hip, stride 2 / fused shortcut / 1x1 ----
    _c("pp-s2-2x2", PP, "conv", 1, 2, 2, 64, 128, stride=2, tune=(1, -1, -1), query=("conv3x3s2_pp", (2,)), key="conv3x3s2_pp_kernel<7,4,1>"),
    _c("pp-s2-8x6", PP, "conv", 4, 8, 6, 32, 128, stride=2, res=True, tune=(1, -1, -1), query=("conv3x3s2_pp", (2,)), key="conv3x3s2_pp_kernel<7,4,1>"),
    _c("pp-shortcut-3x5", PP, "ds", 1, 3, 5, 256, 128, ds=(256, 2), tune=(1, -1, -1), query=("conv3x3_pp_ds", (1, 2)), key="conv3x3_pp_kernel<7,4,5,1,DS>"),
    _c("pp-shortcut-10x6", PP, "ds", 4, 10, 6, 64, 128, ds=(32, 2), act=ACT_NONE, tune=(1, -1, -1), query=("conv3x3_pp_ds", (1, 2)), key="conv3x3_pp_kernel<7,4,5,1,DS>"),
    _c("pp1x1-layout1", PP, "conv", 3, 14, 14, 256, 256, k=1, tune=(1, -1, 256), query=("conv1x1_pp", (1,)), key="conv1x1_pp_kernel<7,2,1>"),
    _c("pp1x1-layout2-s2", PP, "conv", 2, 28, 28, 128, 256, k=1, stride=2, tune=(1, -1, 128), query=("conv1x1_pp", (2,)), key="conv1x1_pp_kernel<7,4,1>"),
    _c("pp1x1-layout3", PP, "conv", 637, 1, 1, 2048, 512, k=1, res=True, act=ACT_NONE, tune=(1, -1, 1282), query=("conv1x1_pp", (3,)), key="conv1x1_pp_kernel<7,2,2>"),
    _c("pp1x1-5ksteps", PP, "conv", 4, 13, 9, 160, 640, k=1, tune=(1, -1, 1282), query=("conv1x1_pp", (2,)), key="conv1x1_pp_kernel<7,4,1>"),
    # ---- fused 2x2 max-pool (default planning) ----
    _c("pool2-generic", IG, "pool2", 5, 6, 6, 64, 64, query=("pool2_form", (1,)), key="conv_igemm_kernel<256,3,1,POOL>"),
    _c("pool2-wave-c32", IG, "pool2", 5, 8, 24, 32, 64, query=("pool2_form", (2,)), key="conv3x3_c64_wave_kernel<1,POOL,EARLY>"),
    _c("pool2-wave-c64", IG, "pool2", 3, 16, 8, 64, 192, act=ACT_NONE, query=("pool2_form", (2,)), key="conv3x3_c64_wave_kernel<2,POOL,EARLY>"),
    _c("pool2-pp-8x8", PP, "pool2", 3, 8, 8, 128, 128, query=("pool2_form", (3,)), key="conv3x3_pp_kernel<7,4,3,1,PL>"),
    _c("pool2-pp-4x4", PP, "pool2", 9, 4, 4, 256, 128, act=ACT_NONE, query=("pool2_form", (3,)), key="conv3x3_pp_kernel<7,4,3,1,PL>"),
    _c("pool2-pp-2x2", PP, "pool2", 33, 2, 2, 128, 128, query=("pool2_form", (3,)), key="conv3x3_pp_kernel<7,4,5,1,PL>"),
    # ---- Cin = 3 ----
    _c("c3-pool2-10x14", SC, "c3pool2", 3, 10, 14, 3, 32),
    _c("c3-pool2-2x2", SC, "c3pool2", 1, 2, 2, 3, 32),
    _c("c3-7x7s2", SC, "c3", 3, 20, 12, 3, 64, k=7, stride=2),
    _c("c3-3x3", SC, "c3", 3, 20, 12, 3, 32),
    _c("stem-pool3-odd", ST, "stem3", 2, 61, 37, 3, 64, k=7, stride=2),
    _c("stem-pool2-odd", ST, "stem2", 2, 61, 37, 3, 64, k=7, stride=2),
    _c("stem-s2d-pool3", S2D, "stem3", 2, 61, 36, 3, 64, k=7, stride=2),
    _c("stem-s2d-pool2", S2D, "stem2", 2, 61, 36, 3, 64, k=7, stride=2),
    _c("stem-u8-pool3", S2D, "stem3u8", 2, 61, 36, 3, 64, k=7, stride=2),
    _c("stem-u8-pool2", S2D, "stem2u8", 2, 61, 36, 3, 64, k=7, stride=2),
]

# GELU is not exact: these run in the bound family only, one per epilogue that implements the activation
GELU_CASES = [
    _c("gelu-wave", IG, "conv", 1, 8, 8, 64, 64, act=ACT_GELU, tune=PP_OFF, query=("conv3x3_pp", (0,)), key="conv3x3_c64_wave_kernel<2,EARLY>"),
    _c("gelu-g1-3x3", IG, "conv", 2, 13, 17, 128, 128, res=True, act=ACT_GELU, tune=PP_OFF, query=("conv3x3_pp", (0,)), key="conv3x3_fast_kernel<>"),
    # (the 128-channel tile forced: left to the planner this shape takes split-K and repeats gelu-pp-splitk)
    _c("gelu-pp-3x3", PP, "conv", 2, 13, 17, 128, 128, res=True, act=ACT_GELU, tune=(1, -1, 128), query=("conv3x3_pp", (2,)), key="conv3x3_pp_kernel<7,4,5,1>"),
    _c("gelu-pp-splitk", PP, "conv", 2, 20, 12, 64, 128, act=ACT_GELU, tune=(1, -1, 1282), query=("conv3x3_pp", (3,)), key="conv3x3_pp_kernel<7,2,6,2>"),
    _c("gelu-pp-s2", PP, "conv", 4, 8, 6, 32, 128, stride=2, act=ACT_GELU, tune=(1, -1, -1), query=("conv3x3s2_pp", (2,)), key="conv3x3s2_pp_kernel<7,4,1>"),
    _c("gelu-pp-shortcut", PP, "ds", 4, 10, 6, 64, 128, ds=(32, 2), act=ACT_GELU, tune=(1, -1, -1), query=("conv3x3_pp_ds", (1, 2)), key="conv3x3_pp_kernel<7,4,5,1,DS>"),
    _c("gelu-pp1x1", PP, "conv", 9, 7, 7, 1024, 384, k=1, res=True, act=ACT_GELU, tune=(1, -1, -1), query=("conv1x1_pp", (1, 2, 3)), key="conv1x1_pp_kernel<7,2,2>"),
]

# ---- the census table: one sharp case for every instantiation the tables above do not reach (`test_conv_census_cpu.py` holds the
# union of keys against `ops.conv_plan_keys()`), and the two shipped options no case above switches on: FRMAP_PP_IM (DMA issued
# between the MFMAs) and FRMAP_PP_PITCH (conflict-free halo pitch).  Shapes: the smallest that reach the key with two tiles or a
# partial last one where the kernel has tiles; every entry names its key, which `launch_case` asserts on the device.
P3 = "conv3x3_pp_kernel"
_B256, _B128, _SPLITK = (1, -1, 256), (1, -1, 128), (1, -1, 1282)
CENSUS_CASES = [
    # 224 px x 256 ch with more than three halo pieces: 5x5 maps, 8 images in a 200-pixel tile (8 x 7 + 3 halo rows of 7 pixels)
    _c("cx-pp251", PP, "conv", 9, 5, 5, 128, 256, res=True, tune=_B256, ri=0, query=("conv3x3_pp", (1,)), key=P3 + "<7,2,5,1>"),
    _c("cx-pp251-ri", PP, "conv", 9, 5, 5, 128, 256, res=True, tune=_B256, ri=1, query=("conv3x3_pp", (1,)), key=P3 + "<7,2,5,1,RI>"),
    _c("cx-pp251-ds", PP, "ds", 9, 5, 5, 128, 256, ds=(64, 2), tune=_B256, query=("conv3x3_pp_ds", (1,)), key=P3 + "<7,2,5,1,DS>"),
    _c("cx-pp251-pl", PP, "pool2", 20, 4, 4, 128, 256, query=("pool2_form", (3,)), key=P3 + "<7,2,5,1,PL>"),
    _c("cx-pp231-pl", PP, "pool2", 5, 8, 8, 128, 256, act=ACT_NONE, query=("pool2_form", (3,)), key=P3 + "<7,2,3,1,PL>"),
    # the same operands as cx-pp251 in the 448 px x 128 ch layout
    _c("cx-pp451-5x5", PP, "conv", 9, 5, 5, 128, 256, res=True, tune=_B128, ri=0, query=("conv3x3_pp", (2,)), key=P3 + "<7,4,5,1>"),
    _c("cx-pp431-ri", PP, "conv", 7, 5, 3, 32, 128, res=True, act=ACT_NONE, tune=(1, -1, -1), ri=1, query=("conv3x3_pp", (2,)), key=P3 + "<7,4,3,1,RI>"),
    # split-K with four halo pieces, where interleaved reads are honoured (at six the planner declines them: pp-splitk-ri1)
    _c("cx-splitk4-ri0", PP, "conv", 9, 14, 14, 256, 256, tune=(1, 196, 1282), ri=0, query=("conv3x3_pp", (3,)), key=P3 + "<7,2,4,2>"),
    _c("cx-splitk4-ri1", PP, "conv", 9, 14, 14, 256, 256, tune=(1, 196, 1282), ri=1, query=("conv3x3_pp", (3,)), key=P3 + "<7,2,4,2,RI>"),
    # stride 2
    _c("cx-s2pp-721", PP, "conv", 4, 8, 6, 32, 256, stride=2, res=True, tune=(1, -1, -1), query=("conv3x3s2_pp", (1,)), key="conv3x3s2_pp_kernel<7,2,1>"),
    _c("cx-s2pp-742", PP, "conv", 3, 16, 16, 32, 128, stride=2, tune=(1, -1, -1), query=("conv3x3s2_pp", (2,)), key="conv3x3s2_pp_kernel<7,4,2>"),
    # first generation: the 128-pixel generic tiles (rows too wide for 256 pixels' halo) and the two-chunk 1x1 stage
    _c("cx-igemm128", IG, "conv", 1, 1, 220, 32, 64, tune=PP_OFF, query=("conv3x3_pp", (0,)), key="conv_igemm_kernel<128,3,1>"),
    _c("cx-igemm128-s2", IG, "conv", 1, 7, 300, 32, 64, stride=2, act=ACT_NONE, tune=PP_OFF, query=("conv3x3s2_pp", (0,)), key="conv_igemm_kernel<128,3,2>"),
    _c("cx-igemm128-pool", IG, "pool2", 1, 4, 120, 96, 64, query=("pool2_form", (1,)), key="conv_igemm_kernel<128,3,1,POOL>"),
    _c("cx-1x1-cks2", IG, "conv", 4, 13, 9, 192, 128, k=1, res=True, tune=PP_OFF, query=("conv1x1_pp", (0,)), key="conv1x1_kernel<2>"),
    # the wave kernel's start-up form 0 (nothing resident early) on the exact family, all three instantiations
    _c("cx-wave-late", IG, "conv", 3, 16, 24, 64, 128, res=True, tune=PP_OFF, wstart=0, query=("conv3x3_pp", (0,)), key="conv3x3_c64_wave_kernel<2>"),
    _c("cx-wave-late-pool-c32", IG, "pool2", 5, 8, 24, 32, 64, wstart=0, query=("pool2_form", (2,)), key="conv3x3_c64_wave_kernel<1,POOL>"),
    _c("cx-wave-late-pool-c64", IG, "pool2", 3, 16, 8, 64, 192, act=ACT_NONE, wstart=0, query=("pool2_form", (2,)), key="conv3x3_c64_wave_kernel<2,POOL>"),
    # FRMAP_PP_IM = 1 on every (WM, NHP, KS) layout: the shapes of pp-bn256-ri0, cx-pp251, pp-1chunk, pp-bn128-ri0, cx-splitk4-ri0, pp-splitk-ri0
    _c("cx-im-231", PP, "conv", 5, 14, 14, 256, 256, res=True, tune=_B256, ri=0, im=1, query=("conv3x3_pp", (1,)), key=P3 + "<7,2,3,1,IM>"),
    _c("cx-im-251", PP, "conv", 9, 5, 5, 128, 256, res=True, tune=_B256, ri=0, im=1, query=("conv3x3_pp", (1,)), key=P3 + "<7,2,5,1,IM>"),
    _c("cx-im-431", PP, "conv", 7, 5, 3, 32, 128, res=True, act=ACT_NONE, tune=(1, -1, -1), ri=0, im=1, query=("conv3x3_pp", (2,)), key=P3 + "<7,4,3,1,IM>"),
    _c("cx-im-451", PP, "conv", 5, 14, 14, 256, 256, res=True, tune=_B128, ri=0, im=1, query=("conv3x3_pp", (2,)), key=P3 + "<7,4,5,1,IM>"),
    _c("cx-im-242", PP, "conv", 9, 14, 14, 256, 256, tune=(1, 196, 1282), ri=0, im=1, query=("conv3x3_pp", (3,)), key=P3 + "<7,2,4,2,IM>"),
    _c("cx-im-262", PP, "conv", 2, 20, 12, 64, 128, tune=_SPLITK, ri=0, im=1, query=("conv3x3_pp", (3,)), key=P3 + "<7,2,6,2,IM>"),
    # FRMAP_PP_PITCH = 1: Wp grows from Wi + 2 to the next value that is Wi (mod 8), and the halo with it.  NHP class after / before:
    # All three on 14x14 maps in 196-pixel tiles, Wp 16 -> 22, 16 halo rows: 16 KB -> 22 KB.  NHP class before / after:
    #   cx-pitch-plain   224 px x 256 ch, 8 KB pieces: 3 / 3        (the twin without it: pp-bn256-ri0)
    #   cx-pitch-ds      the same layout with the fused shortcut: 3 / 3   (cx-pp231-ds)
    #   cx-pitch-splitk  split-K, 4 KB pieces: 4 / 6                (cx-splitk4-ri0; on 20x12 maps, 6 before, a seventh piece does not
    #                    exist and the planner leaves split-K)
    _c("cx-pitch-plain", PP, "conv", 5, 14, 14, 256, 256, res=True, tune=_B256, ri=0, pitch=1, query=("conv3x3_pp", (1,)), key=P3 + "<7,2,3,1>"),
    _c("cx-pitch-ds", PP, "ds", 3, 14, 14, 128, 256, ds=(64, 2), tune=_B256, pitch=1, query=("conv3x3_pp_ds", (1,)), key=P3 + "<7,2,3,1,DS>"),
    _c("cx-pitch-splitk", PP, "conv", 9, 14, 14, 256, 256, tune=(1, 196, 1282), ri=0, pitch=1, query=("conv3x3_pp", (3,)), key=P3 + "<7,2,6,2>"),
    # reached before by the Gaussian operands of test_conv_fill_gpu.py only: the shortcut form with three halo pieces and the stride-2
    # layouts of 14x14 and 28x28 output maps
    _c("cx-pp231-ds", PP, "ds", 3, 14, 14, 128, 256, ds=(64, 2), tune=_B256, query=("conv3x3_pp_ds", (1,)), key=P3 + "<7,2,3,1,DS>"),
    _c("cx-s2pp-722", PP, "conv", 3, 28, 28, 64, 256, stride=2, res=True, tune=_B256, query=("conv3x3s2_pp", (1,)), key="conv3x3s2_pp_kernel<7,2,2>"),
    _c("cx-s2pp-744", PP, "conv", 2, 56, 56, 32, 128, stride=2, act=ACT_NONE, tune=_B128, query=("conv3x3s2_pp", (2,)), key="conv3x3s2_pp_kernel<7,4,4>"),
]

# linear_mfma: M, K, N, act, residual, split-K expected.  Split-K is taken when min(384 / tiles, (K / 32) / 4) >= 2
# (`linear_ksplit`): at these tile counts from K = 256 on (8 chunks); K = 224 (7 chunks) is the largest K that does not split.
LinCase = namedtuple("LinCase", "name M K N act res split")
LINEAR_CASES = [
    LinCase("linear-res", 5, 512, 256, ACT_NONE, True, True),
    LinCase("linear-smallest-splitk", 5, 256, 256, ACT_RELU, False, True),
    LinCase("linear-no-split", 5, 224, 256, ACT_RELU, True, False),
    LinCase("linear-gelu-splitk", 5, 512, 256, ACT_GELU, True, True),      # bound family only (`splitk_finalize_kernel`'s own GELU)
]
LINEAR_FILE = IG

# pairs of cases that run the same operands on two generations, or with and without interleaved fragment reads: the exact family
# requires their outputs to agree bit for bit
# (pp-splitk-ri0 / -ri1: the planner declines interleaved reads at six halo pieces, so both run conv3x3_pp_kernel<7,2,6,2> - their
#  keys say so - and the pair holds a kernel to itself; the pair on which the request is honoured is cx-splitk4-ri0 / -ri1)
SAME_BITS = [("pp-bn128-ri0", "pp-bn128-ri1"), ("pp-bn256-ri0", "pp-bn256-ri1"), ("pp-bn128-ri0", "pp-bn256-ri0"),
             ("pp-splitk-ri0", "pp-splitk-ri1"), ("pp-px37-bn256", "pp-px37-splitk"), ("g1-shortcut-3x5", "pp-shortcut-3x5"),
             ("g1-shortcut-10x6", "pp-shortcut-10x6"), ("1x1-gather-c128", "pp1x1-layout2-s2"), ("1x1-stage1", "pp1x1-5ksteps")]
# the census pairs: asserted bit-identical on the exact operands and on Gaussian ones.  The planner's comments say none of these
# changes the k order of an output element: DMA issue order (IM), halo pitch, read placement (RI), pixel split against pixel split.
CENSUS_SAME_BITS = [
    ("pp-bn256-ri0", "cx-im-231"), ("cx-pp251", "cx-im-251"), ("pp-1chunk", "cx-im-431"), ("pp-bn128-ri0", "cx-im-451"),
    ("cx-splitk4-ri0", "cx-im-242"), ("pp-splitk-ri0", "cx-im-262"),
    ("pp-bn256-ri0", "cx-pitch-plain"), ("cx-pp231-ds", "cx-pitch-ds"), ("cx-splitk4-ri0", "cx-pitch-splitk"),
    ("cx-splitk4-ri0", "cx-splitk4-ri1"), ("cx-pp251", "cx-pp451-5x5"),
]

# one subnormal-weight case per kernel file (fp16), and one on an instantiation of conv_pp.hip the census table added
SUBNORMAL_CASES = ["g1-c512-7x7", "pp-splitk-res", "c3-3x3", "stem-pool3-odd", "stem-s2d-pool3", "cx-pp251-ds"]


def case_by_name(name):
    return next(c for c in CONV_CASES + GELU_CASES + CENSUS_CASES if c.name == name)


def exact_n_nz(case):
    """nonzeros per output channel: 200 (S peaks near 165), 120 + 120 with a fused shortcut, dense for Cin = 3 (147 + 8)."""
    return 120 if case.ds is not None else 200


def case_seed(case):
    """A table entry's seed by its position; a case from another table (`big_cases.py`) by a checksum of its name."""
    names = [c.name for c in CONV_CASES + GELU_CASES]
    if case.name in names:
        return 7000 + 13 * names.index(case.name)
    return 9000 + 13 * (zlib.crc32(case.name.encode()) % 4096)


def case_pad(case):
    return 3 if case.k == 7 else case.k // 2


def exact_case_operands(case):
    if case.Cin == 3:      # dense +-1 weights: S <= 147 + 8  (the uint8 entry's x comes from `u8_operands`)
        return exact_operands(case_seed(case), case.B, case.H, case.W, 3, case.Cout, case.k, case.stride, case_pad(case), False, 7 * 7 * 3)
    return exact_operands(case_seed(case), case.B, case.H, case.W, case.Cin, case.Cout, case.k, case.stride, case_pad(case),
                          case.res, exact_n_nz(case), case.ds)


def float_case_operands(case, family, dtype):
    return float_operands(family, case_seed(case), case.B, case.H, case.W, case.Cin, case.Cout, case.k, dtype, case.stride,
                          case_pad(case), case.res, case.ds, shift_std=0.3 if case.op.startswith("stem") else 0.1)


def case_reference(case, o):
    """(want, S, act) of a case on operand dict `o`: `want` is the float64 pre-activation, or for a pooled op the pooled
    activation (act then ACT_NONE); NCHW."""
    if case.op == "ds":
        ref, S = conv_shortcut_ref(o["x"], o["w"], o["shift"], o["xd"], o["wd"], case.ds[1])
        return ref, S, case.act
    ref, S = conv_ref(o["x"], o["w"], o["shift"], case.stride, case_pad(case), o.get("r"))
    if case.op in ("pool2", "c3pool2"):
        return pooled(ref, S, case.act, 2, 2, 0) + (ACT_NONE,)
    if case.op.startswith("stem3"):
        return pooled(ref, S, ACT_RELU, 3, 2, 1) + (ACT_NONE,)
    if case.op.startswith("stem2"):
        return pooled(ref, S, ACT_RELU, 2, 2, 0) + (ACT_NONE,)
    return ref, S, case.act


# ------------------------------------------------------------------------------------------------------------------------------
# running a case through the C ABI (GPU)
# ------------------------------------------------------------------------------------------------------------------------------
DEV = "cuda"
U8_MEAN = U8_STD = (1.0 / 255, 1.0 / 255, 1.0 / 255)      # (u / 255 - mean) / std = u - 1 for the bytes 0, 1, 2


def _to_dev(t):
    return t.to(DEV)


def _nhwc(t, dtype, place=_to_dev):
    return place(t.permute(0, 2, 3, 1).contiguous().to(dtype))


def _sync(what):
    """Wait for the launches; a device fault ends the whole session (nothing more is started on a card that has faulted)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        import pytest
        pytest.exit(f"{what}: the GPU reported {e}; stopping the session", returncode=3)


CONV_OPS = ("conv", "ds", "pool2")      # the ops the conv planner plans (`ops.conv_plan_key`)


def case_ds(case):
    """(dsH, dsW, dsCin, ds_stride) of the shortcut's input map as `exact_operands` / `float_operands` build it."""
    dsC, sd = case.ds
    return (case.H - 1) * sd + 1 + (sd - 1), (case.W - 1) * sd + 1 + (sd - 1), dsC, sd


def set_hooks(lib, case):
    """The process-wide hooks of a case; `reset_hooks` in a `finally` takes them back."""
    if case.tune is not None:
        assert lib.frmap_conv_pp_tuning(*case.tune) == 0
    for value, hook in ((case.ri, lib.frmap_conv_pp_ri), (case.im, lib.frmap_conv_pp_im), (case.pitch, lib.frmap_conv_pp_pitch),
                        (case.wstart, lib.frmap_conv_wave_start)):
        if value is not None:
            assert hook(value) == 0


def reset_hooks(lib, case=None):
    """(`frmap_conv_wave_start` only where the case set it: `test_conv_wave_pipeline_gpu.py` sets it around its launches)"""
    lib.frmap_conv_pp_tuning(-1, -1, -1)
    lib.frmap_conv_pp_ri(-1)
    lib.frmap_conv_pp_im(-1)
    lib.frmap_conv_pp_pitch(-1)
    lib.frmap_conv_pp_ds(-1)
    if case is not None and case.wstart is not None:
        lib.frmap_conv_wave_start(-1)


def plan_key(ops, case):
    """`ops.conv_plan_key` of the case's launch under the hooks now in force (needs no GPU)."""
    if case.op == "ds":
        return ops.conv_plan_key(case.B, case.H, case.W, case.Cin, case.Cout, 3, 1, ops.FUSE_SHORTCUT, case_ds(case))
    if case.op == "pool2":
        return ops.conv_plan_key(case.B, case.H, case.W, case.Cin, case.Cout, 3, 1, ops.FUSE_POOL2)
    assert case.op == "conv", case.op
    return ops.conv_plan_key(case.B, case.H, case.W, case.Cin, case.Cout, case.k, case.stride, ops.FUSE_RESIDUAL if case.res else ops.FUSE_NONE)


def planned_key(case):
    """The key of the case's launch under its own hooks, which are reset afterwards: what `launch_case` asserts, without a launch."""
    from frmap_amd import _lib, ops
    lib = _lib.load()
    try:
        set_hooks(lib, case)
        return plan_key(ops, case)
    finally:
        reset_hooks(lib, case)


def query_path(lib, ops, case):
    """The answer of the case's layout / form query under the tuning now in force."""
    B, H, W, Cin, Cout = case.B, case.H, case.W, case.Cin, case.Cout
    name = case.query[0]
    if name == "conv3x3_pp":
        return lib.frmap_conv3x3_pp_layout(B, H, W, Cin, Cout)
    if name == "conv3x3s2_pp":
        return lib.frmap_conv3x3s2_pp_layout(B, H, W, Cin, Cout)
    if name == "conv1x1_pp":
        return lib.frmap_conv1x1_pp_layout(B, H, W, Cin, Cout, case.stride)
    if name == "conv3x3_pp_ds":
        dsC, sd = case.ds
        return lib.frmap_conv3x3_pp_ds_layout(B, H, W, Cin, Cout, (H - 1) * sd + 1 + (sd - 1), (W - 1) * sd + 1 + (sd - 1), dsC, sd)
    if name == "pool2_form":
        form = ops.conv_pool2_form(B, H, W, Cin, Cout)
        assert (form == 3) == (lib.frmap_conv3x3_pp_pool_layout(B, H, W, Cin, Cout) == 1 and Cin >= 128), (case.name, form)
        return form
    raise ValueError(name)


def device_operands(case, o, dtype, place=None):
    """The operands of a case on the device, as its launch takes them (`place`: how a CPU tensor gets there): the shift, the NHWC
    activations (`x`, `r`, `xd`; `x4` for the Cin = 3 kernels; the stems' fp32 NCHW `x` or uint8 `u8` with `mean`, `std`) and the
    packed weights (`wpk`, `wdpk`).  Every activation keeps the batch as its first dimension."""
    place = place or _to_dev
    from frmap_amd import ops
    d = {"sh": place(o["shift"].float())}
    if case.op in ("conv", "ds", "pool2"):
        d["x"], d["wpk"] = _nhwc(o["x"], dtype, place), ops.pack_conv_weight(place(o["w"].float()), dtype)
        if case.op == "conv" and o.get("r") is not None:
            d["r"] = _nhwc(o["r"], dtype, place)
        if case.op == "ds":
            d["xd"] = _nhwc(o["xd"], dtype, place)
            d["wdpk"] = ops.pack_conv_weight(place(o["wd"].float()), dtype)
    elif case.op in ("c3", "c3pool2"):
        x4 = torch.zeros(tuple(o["x"].shape[i] for i in (0, 2, 3)) + (4,), dtype=dtype)
        x4[..., :3] = o["x"].permute(0, 2, 3, 1).to(dtype)
        d["x4"], d["wpk"] = place(x4), ops.pack_conv_weight_c3(place(o["w"].float()), dtype)
    elif case.op in ("stem3", "stem2"):
        d["wpk"] = ops.pack_conv_weight_c3(place(o["w"].float()), dtype)
        d["x"] = place(o["x"].float())
    elif case.op in ("stem3u8", "stem2u8"):
        d["wpk"] = ops.pack_conv_weight_c3(place(o["w"].float()), dtype)
        d["u8"], d["mean"], d["std"] = place(o["u8"]), o["mean"], o["std"]
    else:
        raise ValueError(case.op)
    return d


def launch_case(case, d, dtype, also_unfused=False, sync=True):
    """Launch the case's kernel on the device operands `d` (`device_operands`; `case.B` is the batch of the tensors in `d`) and
    return the output as it lies on the device, NHWC in `dtype` (`also_unfused`: for the fused-pool ops, the (fused, two-launch)
    outputs).  Asserts the path the case is about where a query exists, waits for the launches (`sync=False`: does not - the
    stream tests launch a case while its operands are late, or into a graph) and restores the process-wide tuning hooks."""
    from frmap_amd import _lib, ops
    lib = _lib.load()
    try:
        set_hooks(lib, case)
        if case.query is not None:
            got = query_path(lib, ops, case)
            assert got in case.query[1], (case.name, case.query[0], "answers", got, "wanted", case.query[1])
        if case.key is not None:       # the instantiation this launch dispatches, on this device's CU count
            got = plan_key(ops, case)
            assert got == case.key, (case.name, "launches", got, "the table says", case.key)
        sh, wpk = d["sh"], d["wpk"]
        y2 = None
        if case.op == "conv":
            y = ops.conv_igemm(d["x"], wpk, sh, case.Cout, case.k, case.stride, case_pad(case), case.act, d.get("r"))
        elif case.op == "ds":
            xd = d["xd"]
            assert ops.conv_ds_supported(case.B, case.H, case.W, case.Cin, case.Cout, xd.shape[1], xd.shape[2], case.ds[0], case.ds[1])
            y = ops.conv_igemm_ds(d["x"], wpk, sh, case.Cout, xd, d["wdpk"], case.ds[1], case.act)
        elif case.op == "pool2":
            y = ops.conv_igemm_pool2(d["x"], wpk, sh, case.Cout, case.act)
            if also_unfused:
                y2 = ops.maxpool(ops.conv_igemm(d["x"], wpk, sh, case.Cout, 3, 1, 1, case.act), 2, 2, 0)
        elif case.op == "c3":
            y = ops.conv_small_cin(d["x4"], wpk, sh, case.Cout, case.k, case.stride, case_pad(case), True)
        elif case.op == "c3pool2":
            y = ops.conv_small_cin_pool2(d["x4"], wpk, sh, case.Cout, True)
            if also_unfused:
                y2 = ops.maxpool(ops.conv_small_cin(d["x4"], wpk, sh, case.Cout, 3, 1, 1, True), 2, 2, 0)
        elif case.op in ("stem3", "stem2"):
            y = ops.stem7x7_maxpool(d["x"], wpk, sh, dtype, pool3=case.op == "stem3")
        elif case.op in ("stem3u8", "stem2u8"):
            y = ops.stem7x7_maxpool_u8(d["u8"], wpk, sh, d["mean"], d["std"], dtype, pool3=case.op == "stem3u8")
        else:
            raise ValueError(case.op)
        if sync:
            _sync(case.name)
        return (y, y2) if also_unfused and y2 is not None else y
    finally:
        reset_hooks(lib, case)


def run_case(case, o, dtype, also_unfused=False, place=None):
    """Launch the case's kernel on operand dict `o` (values `dtype` represents exactly) and return the output as a CPU NCHW tensor
    in `dtype`.  Asserts the path the case is about where a query exists, and restores the process-wide tuning hooks.
    `also_unfused`: for the fused-pool ops, returns (fused, two-launch) outputs.  `place`: how a CPU operand reaches the device
    (None: a plain copy; `guard.Guard.place` puts it between guard bands)."""
    y = launch_case(case, device_operands(case, o, dtype, place), dtype, also_unfused)
    if isinstance(y, tuple):
        return tuple(t.cpu().permute(0, 3, 1, 2) for t in y)
    return y.cpu().permute(0, 3, 1, 2)


def u8_operands(case, dtype, exact):
    """(bytes [B,H,W,3], mean, std, x [B,3,H,W]) of the uint8 stem entry.  `x` is what the entry's per-channel table makes of the
    bytes: `ops.normalize_u8` rounded to `dtype` (the header promises the same rounding; `test_kernels_gpu.py` checks the two entries
    bit for bit).  exact: bytes 0 / 1 / 2 under mean = std = 1 / 255, asserted to come out as -1 / 0 / 1; else every byte value under
    the ImageNet statistics."""
    from frmap_amd import ops
    g = torch.Generator().manual_seed(case_seed(case) + 5)
    u8 = torch.randint(0, 3 if exact else 256, (case.B, case.H, case.W, 3), generator=g).to(torch.uint8)
    mean, std = (U8_MEAN, U8_STD) if exact else ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    x = ops.normalize_u8(u8.to(DEV), mean, std)[0].to(dtype).cpu()
    if exact:
        assert torch.equal(x.double(), u8.permute(0, 3, 1, 2).double() - 1.0), "bytes 0 / 1 / 2 did not normalise to -1 / 0 / 1"
    return u8, mean, std, x


def gpu_operands(case, family, dtype):
    """Operand dict of a case for `run_case`: family 'exact' or one of `float_operands`'; the uint8 entry's image replaces x."""
    o = exact_case_operands(case) if family == "exact" else float_case_operands(case, family, dtype)
    if case.op.endswith("u8"):
        o["u8"], o["mean"], o["std"], o["x"] = u8_operands(case, dtype, family == "exact")
    return o


def run_linear(lc, o, dtype, place=None):
    """`ops.linear_mfma` on operands x [M,K], w [N,K], shift, r; asserts that split-K is (not) taken as the case says.
    `place`: as `run_case`."""
    place = place or _to_dev
    from frmap_amd import _lib, ops
    lib = _lib.load()
    assert (lib.frmap_linear_mfma_workspace_bytes(lc.M, lc.K, lc.N) > 0) == lc.split, (lc.name, "split-K")
    if lc.name == "linear-smallest-splitk":
        assert lib.frmap_linear_mfma_workspace_bytes(lc.M, lc.K - 32, lc.N) == 0, "a smaller K splits"
    wpk = ops.pack_conv_weight(place(o["w"].float().view(lc.N, lc.K, 1, 1)), dtype)
    r = place(o["r"].to(dtype)) if o.get("r") is not None else None
    y = ops.linear_mfma(place(o["x"].to(dtype)), wpk, place(o["shift"].float()), lc.N, lc.act, r)
    _sync(lc.name)
    return y.cpu()


def linear_operands(lc, family, dtype):
    """Operands of a linear case as [M, K] / [N, K] / [M, N] tensors; family 'exact' or one of `float_operands`'."""
    seed = 7900 + 17 * [c.name for c in LINEAR_CASES].index(lc.name)
    if family == "exact":
        o = exact_operands(seed, lc.M, 1, 1, lc.K, lc.N, 1, res=lc.res)
    else:
        o = float_operands(family, seed, lc.M, 1, 1, lc.K, lc.N, 1, dtype, res=lc.res)
    return {"x": o["x"].reshape(lc.M, lc.K), "w": o["w"].reshape(lc.N, lc.K), "shift": o["shift"],
            "r": o["r"].reshape(lc.M, lc.N) if o["r"] is not None else None}
