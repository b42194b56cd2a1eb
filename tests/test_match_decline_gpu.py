"""GPU: a prepared gallery whose shape the split-fp16 match GEMM declines is answered by every packed entry point exactly as by
its unpacked twin.  D = 5472 is the smallest multiple of 32 with K = 3 D > 16384; G >= `ops.MATCH_MFMA_MIN_G`, so ``prepared``
reaches `frmap_match_top1_packed`, `frmap_match_topk_packed` and `frmap_verify_counts_packed`.

Bar: with and without ``prepared`` bit-identical; indices / counts equal to the numpy references (`match_cases.float64_first_min`,
`ref_topk`, `ref_verify_counts`) with no tie allowance; |dist - ref| <= 2e-6 + 1e-6 * ref."""
import numpy as np
import pytest
import torch

from frmap_amd import evaluate, ops

import match_cases as mc
from test_match_topk_cpu import ref_topk
from test_verify_cpu import ref_verify_counts

pytestmark = pytest.mark.gpu
DEV = "cuda"
G, D = 520, 5472


@pytest.fixture(scope="module")
def case():
    probes, gal, notes = mc.build_case(G, D, "unit", 5472)
    labels = np.arange(G, dtype=np.int32) % 97                   # identity mode: five or six rows per label
    # a probe made from gallery row r carries r's label (its near-duplicate pairs are genuine), the others a label of their own
    probe_labels = np.array([labels[m] if m >= 0 else 1000 + p for p, (_, _, m) in enumerate(notes)], np.int32)
    return probes, gal, labels, probe_labels


def _dist_ok(dist, ref):
    dist = np.asarray(dist, np.float64)
    fin = np.isfinite(ref)
    return bool(np.all(np.isinf(dist[~fin])) and np.all(np.abs(dist[fin] - ref[fin]) <= 2e-6 + 1e-6 * ref[fin]))


@pytest.mark.parametrize("op", ["top1", "topk_entry", "topk_identity", "verify"])
def test_declined_pack_answers_as_unpacked(case, op):
    probes, gal, labels, probe_labels = case
    assert 3 * D > 16384 and ops.wants_pack(G, D)
    pd, gd = probes.to(DEV), gal.to(DEV)
    prep = ops.match_prepare(gd)
    if op == "top1":
        plain, packed = ops.match_top1(pd, gd), ops.match_top1(pd, gd, prepared=prep)
        assert all(torch.equal(a, b) for a, b in zip(plain, packed))
        ref = [mc.float64_first_min(probes[p:p + 1], gal)[:2] for p in range(probes.shape[0])]   # (one probe at a time: memory)
        assert plain[0].cpu().long().tolist() == [int(i) for i, _ in ref]
        assert _dist_ok(plain[1].cpu().numpy(), np.array([float(d) for _, d in ref]))
    elif op.startswith("topk"):
        k, lab = 5, (torch.from_numpy(labels).to(DEV) if op == "topk_identity" else None)
        plain, packed = ops.match_topk(pd, gd, k, labels=lab), ops.match_topk(pd, gd, k, labels=lab, prepared=prep)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(plain, packed))
        ri, rd, rl = ref_topk(probes.numpy(), gal.numpy(), k, labels if lab is not None else None)
        assert np.array_equal(plain[0].cpu().long().numpy(), ri)
        assert _dist_ok(plain[1].cpu().numpy(), rd)
        if lab is not None:
            assert np.array_equal(plain[2].cpu().long().numpy(), rl)
    else:
        t = np.unique(np.concatenate((evaluate.default_thresholds(torch.cat((probes, gal)), n=256),
                                      np.geomspace(1e-6, 1e-2, 24).astype(np.float32))))   # (+ the near-duplicate separations)
        la, lb = torch.from_numpy(probe_labels).to(DEV), torch.from_numpy(labels).to(DEV)
        plain, packed = ops.verify_counts(pd, la, t, gd, lb), ops.verify_counts(pd, la, t, gd, lb, prepared=prep)
        assert torch.equal(plain, packed)
        ref = ref_verify_counts(probes.numpy(), probe_labels, t, gal.numpy(), labels)
        assert ref[0, -1] > 0 and np.array_equal(plain.cpu().numpy(), ref)
