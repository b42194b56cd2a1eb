"""Shared inputs of the matcher's magnitude-range tests (`test_match_range_cpu.py`, `test_match_range_gpu.py`): galleries and probes
whose rows are unit rows scaled by powers of two from the smallest fp32 subnormal to 2^100, alone and mixed in one call.

Every element is a finite fp32 value or zero, every exact distance ((a - g) + 1e-6 in fp32, squares summed in float64) is finite and
its fp32 cast is finite: the documented answer lists every row.  What the ladder straddles:
  -149 .. -126   subnormal elements and the first normal ones
  -115 / -114 / -113   the cut of the split-fp16 row scale (csrc/match_scale_rule.h: 2^-113; an unclamped 2^(14 - e) overflows below)
  62 .. 66       the overflow of the fp32 squared norm (unit rows: 2^64), where the expanded distance has no finite bound
  100            the top: the fp32 difference of two elements and the fp32 cast of the distance both stay finite
"""
from collections import namedtuple

import numpy as np
import torch

from frmap_amd import synth

import match_cases as mc

LADDER = [-149, -140, -127, -126, -120, -115, -114, -113, -64, -20, 0, 20, 62, 63, 64, 66, 100]
SPLIT_LADDER = [e for e in LADDER if e <= -64 or e >= 20]        # no mid-range row is nearest to everything small
ZERO = None                                                        # the exponent class of an all-zero row

# Verification thresholds: strictly ascending fp32.  2^-20 = 9.5e-7 lies below every distance (eps keeps two rows at least
# sqrt(D) 1e-6 - |a - g| apart, and |a - g| is either below 2^-19 = 1.9e-6 or of the order of a unit row or more);
# 8e-6 IS the distance of an exact tie at D = 64 (sqrt(64 (1e-6f)^2) = 8 x 1e-6f, exact) and 8.1e-6 lies just above it; 1.2e-5 lies
# above the tie at D = 128 (1.13e-5); 1 and 1.5 straddle the unit rows (sqrt 2); 2^20 .. 2^101 straddle the big classes; 3e38 takes all.
THRESHOLDS = [2.0 ** -20, 8e-6, 8.1e-6, 1.2e-5, 1.0, 1.5, 2.0 ** 20, 2.0 ** 62, 2.0 ** 65, 2.0 ** 67, 2.0 ** 101, 3e38]
RADIUS_THRESHOLDS = [2e-5, 1.5, 2.0 ** 65, 2.0 ** 101]

# (G, D).  (200, 64): three full 64-row slots and a ragged one; (65, 128): one row past a slot; (40, 64): less than a slot.
# The launchers' switch points (csrc/head_match.hip, ops.py):
#   frmap_match_top1      G <= 64: the one-launch small-gallery scan (40); G > 64: the fp32 GEMM + exact finalize (65, 200)
#   frmap_match_topk, frmap_verify_counts, frmap_match_radius (unpacked): the exact scans at every G
#   every *_packed entry: the split-fp16 GEMM at every G > 0 with D % 32 == 0 (frmap_match_gemm_takes); ops takes it from
#   ops.MATCH_MFMA_MIN_G = 512 rows on, which the tests lower to 1
SHAPES = [(200, 64), (65, 128), (40, 64)]

Case = namedtuple("Case", "probes gal labels_p labels_g probe_exp gal_exp")


def f32(x64):
    """float64 -> fp32, rounded once (to a subnormal or zero where the value is that small)."""
    return torch.from_numpy(np.asarray(x64, dtype=np.float64).astype(np.float32))


def _labels(n):
    return torch.arange(n, dtype=torch.int64) % 7


def _laddered(G, D, seed, ladder):
    n = len(ladder)
    unit = synth.unit_rows(seed, G, D, "range_gal").double().numpy()
    gal_exp = [ladder[i % n] for i in range(G)]
    gal = f32(unit * np.array([2.0 ** e for e in gal_exp])[:, None])
    gal[G - 1] = 0.0
    gal_exp[G - 1] = ZERO
    rng = np.random.default_rng(seed + 11)
    fresh = synth.unit_rows(seed + 1, n, D, "range_probe").double().numpy()
    probes, probe_exp = [], []
    for c, e in enumerate(ladder):                      # gallery row c is the first row of exponent class c
        probes.append(gal[c].clone())                                                                 # a bit copy
        probes.append(f32(gal[c].double().numpy() * (1.0 + 2.0 ** -10 * rng.standard_normal(D))))    # near it
        probes.append(f32(fresh[c] * 2.0 ** e))                                                      # a fresh row at that exponent
        probe_exp += [e, e, e]
    probes.append(torch.zeros(D))
    probe_exp.append(ZERO)
    probes = torch.stack(probes).contiguous()
    return Case(probes, gal.contiguous(), _labels(probes.shape[0]), _labels(G), probe_exp, gal_exp)


def mixed(G, D, seed):
    """Gallery row i = unit row i x 2^LADDER[i % 17] (the last row all zero); per exponent a bit copy of a gallery row of that
    exponent, that row x (1 + 2^-10 noise) and a fresh unit row at that exponent; one all-zero probe."""
    return _laddered(G, D, seed, LADDER)


def split(G, D, seed):
    """`mixed` without the exponents -20 and 0: every small or zero probe ties EXACTLY with every small gallery row and the zero row
    (each element of the difference becomes exactly 1e-6f), so the first small row - row 0 - must win."""
    return _laddered(G, D, seed, SPLIT_LADDER)


def uniform(G, D, e, seed):
    """The near-duplicate gallery and probes of `match_cases.build_case` (unit rows), all scaled by 2^e."""
    probes, gal, _ = mc.build_case(G, D, "unit", seed)
    probes, gal = f32(probes.double().numpy() * 2.0 ** e), f32(gal.double().numpy() * 2.0 ** e)
    P = probes.shape[0]
    return Case(probes.contiguous(), gal.contiguous(), _labels(P), _labels(G), [e] * P, [e] * G)


CASE_IDS = ["mixed", "split"] + [f"u{e}" for e in LADDER]


def build(case_id, G, D):
    seed = 5150 + G + D
    if case_id == "mixed":
        return mixed(G, D, seed)
    if case_id == "split":
        return split(G, D, seed)
    return uniform(G, D, int(case_id[1:]), seed)
