"""Shared inputs of the threshold-search tests (`test_match_radius_cpu.py`, `test_match_radius_gpu.py`).

* `clustered`: the `_clustered` recipe of `test_verify_gpu.py` - `ids` unit-norm centres, rows = a centre + Gaussian noise of norm
  ~ `noise`: two rows of one identity lie ~ 1.41 * noise apart, rows of two identities ~ 1.41 apart.
* `near_duplicates`: the near-duplicate gallery of `match_cases.build_case(1000, 512, "unit", 99)` followed by its probes (1 039
  rows): groups at separations 1e-6 ... 1e-3, bit-identical copies, probes equal to / within 1e-5 of a member.
"""
import numpy as np
import torch

from frmap_amd import synth

import match_cases as mc

# (threshold, accepted pairs) of the 3000-row clustered set in self mode, of 4 498 500 pairs
CLUSTERED_3000 = dict(seed=31, n=3000, d=512, ids=375, noise=0.5)
CLUSTERED_3000_ACCEPTED = ((0.7, 4611), (1.0, 12104))
# (threshold, accepted pairs) of `near_duplicates` in self mode; besides these the tests take the 21st-smallest distance (2.26274e-5 =
# sqrt(512) * 1e-6, the distance of bit-identical rows: 22 pairs sit on it) and its fp32 predecessor (0 pairs)
NEAR_DUPLICATES_ACCEPTED = ((1e-4, 162), (2e-3, 270))


def clustered(seed, n, d, ids, noise=0.35):
    rng = np.random.default_rng(seed)
    centres = synth.unit_rows(seed, ids, d, "verify").numpy()
    lab = rng.integers(0, ids, n).astype(np.int32)
    x = centres[lab] + noise / np.sqrt(d) * rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32), lab


def near_duplicates():
    """fp32 [1039, 512]: gallery rows, then the probes."""
    return torch.cat(mc.build_case(1000, 512, "unit", 99)[1::-1]).numpy()
