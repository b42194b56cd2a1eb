"""GPU: exact top-k gallery search (`frmap_match_topk` exact scan, `frmap_match_topk_packed` split-fp16 GEMM with top-R records
+ exact re-score) against the numpy reference of `test_match_topk_cpu.py`.

Bar: indices equal to the reference with no tie or margin allowance; |dist - ref| <= 2e-6 + 1e-6 * ref (the bar of
`test_match_exact_gpu.py`); padding (-1, +inf, -1) exact; packed and unpacked distances bit-equal (the same exact re-score
is behind both, the small-gallery scan of `match_top1` included: it sums its squares in float64 in the same order);
k = 1 in entry mode bit-identical to `ops.match_top1`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from frmap_amd import _lib, matching, ops, synth  # noqa: E402

import match_cases as mc  # noqa: E402
from test_match_topk_cpu import ref_topk  # noqa: E402

DEV = "cuda"
KS = (1, 2, 5, 16, 64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(pd, gd, k, labels=None, packed=False):
    prep = ops.match_prepare(gd) if packed else None
    idx, dist, lab = ops.match_topk(pd, gd, k, labels=labels, prepared=prep)
    return idx.cpu().long().numpy(), dist.cpu(), (lab.cpu().long().numpy() if lab is not None else None)


def _check(probes, gal, ks=KS, labels=None, packed=True, top1=True, what="", monkeypatch=None):
    """Every k, unpacked and (when the shape allows) packed, against the reference; returns nothing, asserts everything."""
    G, D = gal.shape
    kmax = max(ks)
    ref_i, ref_d, ref_l = ref_topk(probes.numpy(), gal.numpy(), kmax, None if labels is None else labels.numpy())
    pd, gd = probes.to(DEV).contiguous(), gal.to(DEV).contiguous()
    ld = labels.to(DEV).to(torch.int32) if labels is not None else None
    paths = [False] + ([True] if packed and G > 0 and D % 32 == 0 else [])
    for k in ks:
        got = {}
        for pk in paths:
            if pk and monkeypatch is not None:
                monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)          # the GEMM path at every gallery size
            idx, dist, lab = _run(pd, gd if G else None, k, ld, pk)
            if monkeypatch is not None:
                monkeypatch.undo()
            ri, rd = ref_i[:, :k], ref_d[:, :k]
            bad = np.argwhere(idx != ri)
            assert bad.size == 0, (what, G, D, k, pk, [(int(p), int(j), int(idx[p, j]), int(ri[p, j])) for p, j in bad[:8]])
            fin = np.isfinite(rd)
            dd = dist.double().numpy()
            assert np.all(np.isinf(dd[~fin]) & (dd[~fin] > 0)), (what, G, D, k, pk)
            err = np.abs(dd[fin] - rd[fin]) - 1e-6 * rd[fin]
            assert err.size == 0 or float(err.max()) <= 2e-6, (what, G, D, k, pk, float(err.max()))
            if labels is not None:
                assert np.array_equal(lab, ref_l[:, :k]), (what, G, D, k, pk)
            got[pk] = dist
            if top1 and k == 1 and labels is None:
                prep = ops.match_prepare(gd) if (pk and G) else None
                if pk and monkeypatch is not None:
                    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
                i1, d1 = ops.match_top1(pd, gd if G else None, prepared=prep)
                if monkeypatch is not None:
                    monkeypatch.undo()
                assert np.array_equal(i1.cpu().long().numpy(), idx[:, 0]) and torch.equal(d1.cpu(), dist[:, 0]), (what, G, D, pk)
        if len(got) == 2:
            assert torch.equal(got[False], got[True]), (what, G, D, k)


@pytest.mark.parametrize("G,D,kind", mc.CASES)
def test_entry_mode_near_duplicates_is_the_reference(G, D, kind, monkeypatch):
    probes, gal, _ = mc.build_case(G, D, kind, 4242 + G + D)
    _check(probes, gal, what=kind, monkeypatch=monkeypatch)


@pytest.mark.parametrize("G", [0, 1, 7, 64, 65, 511, 512, 4097, 10000])
@pytest.mark.parametrize("D", [256, 512])
def test_entry_mode_gallery_sizes(G, D, monkeypatch):
    gal = synth.unit_rows(900 + G, G, D, "tk_gal") if G else torch.zeros((0, D))
    probes = synth.unit_rows(901 + G, 12, D, "tk_probe")
    if G:
        probes[:4] = gal[torch.arange(4) * max(G // 4, 1) % G] + 1e-5 * probes[:4]
    _check(probes, gal, what="sizes", monkeypatch=monkeypatch)


def test_entry_mode_scan_path_d132():
    gal = synth.unit_rows(931, 700, 132, "tk_gal132")
    probes = synth.unit_rows(932, 9, 132, "tk_p132")
    probes[:3] = gal[[5, 300, 699]]
    _check(probes, gal, packed=False, what="D132")


def test_clustered_galleries(monkeypatch):
    D = 256
    gal = synth.unit_rows(941, 1100, D, "tk_cl")
    anchor = gal[70].clone()
    # one identity enrolled 8 times inside the 64-row slot [64, 128) (more than the 4 rows a record lists)
    for j, r in enumerate(range(66, 122, 7)):
        gal[r] = anchor + (j + 1) * 1e-5 * synth.unit_rows(942 + j, 1, D, "tk_n")[0]
    # one identity across a slot boundary (rows 190..193) and across 256-row tiles (rows 255, 256, 511, 512)
    b = gal[600].clone()
    for j, r in enumerate((190, 191, 192, 193, 255, 256, 511, 512)):
        gal[r] = b + (j + 1) * 3e-6 * synth.unit_rows(960 + j, 1, D, "tk_n2")[0]
    # bit-identical duplicate rows: the first k copies, in row order
    c = gal[900].clone()
    for r in (901, 903, 950, 1000, 1001, 1099):
        gal[r] = c
    probes = torch.stack([anchor, b, c, anchor + 1e-6, b + 2e-6, c + 1e-6])
    _check(probes, gal, what="clustered", monkeypatch=monkeypatch)
    idx, _, _ = _run(probes.to(DEV), gal.to(DEV), 7, None, True)
    assert idx[2].tolist() == [900, 901, 903, 950, 1000, 1001, 1099]
    # collapsed gallery: every row equal -> rows 0..k-1
    flat = gal[:1].repeat(700, 1).contiguous()
    for pk in (False, True):
        monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
        idx, dist, _ = _run(probes.to(DEV), flat.to(DEV), 64, None, pk)
        monkeypatch.undo()
        assert (idx == np.arange(64)[None, :]).all(), pk
        assert torch.equal(dist, dist[:, :1].expand_as(dist))


def test_nan_inf_rows_and_k_beyond_gallery(monkeypatch):
    D = 256
    for G in (9, 600):
        gal = synth.unit_rows(971 + G, G, D, "tk_nan")
        gal[1, 3] = float("nan")
        gal[4, 0] = float("inf")
        gal[G - 1] = float("nan")
        probes = synth.unit_rows(972, 5, D, "tk_nanp")
        probes[0] = gal[2]
        _check(probes, gal, ks=(1, 5, 64), what="nan", monkeypatch=monkeypatch)
        monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
        idx, dist, _ = _run(probes.to(DEV), gal.to(DEV), 64, None, G >= 512)
        monkeypatch.undo()
        listed = min(64, G - 3)
        assert (idx[:, listed:] == -1).all() and torch.isinf(dist[:, listed:]).all()
        assert not np.isin(idx, [1, 4, G - 1]).any()


def test_identity_mode_2000_x_5(monkeypatch):
    D, N, E = 512, 2000, 5
    base = synth.unit_rows(981, N, D, "tk_id")
    seps = torch.tensor([1e-6, 1e-5, 1e-4, 1e-3])
    rows, labels = [base], [torch.arange(N)]
    for j in range(E - 1):
        rows.append(base + seps[j] * synth.unit_rows(982 + j, N, D, "tk_idn"))
        labels.append(torch.arange(N))
    gal, lab = torch.cat(rows), torch.cat(labels)
    perm = torch.from_numpy(np.random.default_rng(983).permutation(N * E))
    gal, lab = gal[perm].contiguous(), lab[perm].contiguous()
    probes = torch.cat([base[:6] + 1e-6, base[[100, 1999]], synth.unit_rows(984, 4, D, "tk_idp")])
    _check(probes, gal, ks=(1, 5, 64), labels=lab, what="identity", monkeypatch=monkeypatch)


def test_reference_gallery_compare_faces_topk():
    import json
    z = json.load(open(os.path.join(ROOT, "tests", "golden", "face_references.json")))
    names, emb = z["names"], torch.tensor(z["embeddings"], dtype=torch.float32).reshape(len(z["names"]), -1)
    refs = [{"name": n, "embedding": emb[i:i + 1].to(DEV)} for i, n in enumerate(names)]
    for i in range(len(names)):
        probe = (emb[i] + 0.01 * synth.unit_rows(990 + i, 1, emb.shape[1], "tk_ref")[0]).to(DEV)
        for thresh in (1.0, 0.05, float("inf")):
            name, d, j = matching.compare_faces(probe, refs, thresh)
            lst = matching.compare_faces_topk(probe, refs, thresh, 8)
            if j is None:
                assert lst == []
            else:
                assert lst[0][0] == name and lst[0][2] == j and abs(lst[0][1] - d) <= 2e-6 + 1e-6 * d
                assert [x[1] for x in lst] == sorted(x[1] for x in lst) and all(x[1] <= thresh for x in lst)
            by_name = matching.compare_faces_topk(probe, refs, float("inf"), 64, by="name")
            got = [x[0] for x in by_name]
            assert got.count("random3") == 1 and len(got) == len(set(names)) and len(set(got)) == len(got)
            if j is not None:
                assert by_name[0][2] == j


def test_enrolment_is_seen(monkeypatch):
    D = 256
    g = matching.Gallery([f"id{i}" for i in range(600)], synth.unit_rows(995, 600, D, "tk_en"), DEV)
    new = synth.unit_rows(996, 1, D, "tk_new")[0]
    row = g.append("newbie", new)
    probe = (new + 1e-6).reshape(1, -1).to(DEV)
    idx, _, lab = matching.search_batch(probe, g, 3, by="name")
    assert idx[0, 0].item() == row and g.label_names[lab[0, 0].item()] == "newbie"
    # in-place edit of one row + MatchPack.update_rows
    mat = g.matrix
    mat[17] = new.to(DEV) + 5e-7
    g._pack.update_rows(mat, 17, 18)
    idx, dist, _ = ops.match_topk(probe, mat, 2, prepared=g._pack)
    assert sorted(idx[0].tolist()) == sorted([17, row])


def test_graph_capture_matches_eager():
    D = 512
    gal = synth.unit_rows(1001, 3000, D, "tk_graph").to(DEV)
    prep = ops.match_prepare(gal)
    probes = synth.unit_rows(1002, 64, D, "tk_gp").to(DEV)
    labels = (torch.arange(3000, device=DEV) // 3).to(torch.int32)
    eager = [ops.match_topk(probes, gal, 16, prepared=prep), ops.match_topk(probes, gal, 16, labels=labels, prepared=prep)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.match_topk(probes, gal, 16, prepared=prep)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = [ops.match_topk(probes, gal, 16, prepared=prep), ops.match_topk(probes, gal, 16, labels=labels, prepared=prep)]
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for (ei, ed, el), (gi, gd, gl) in zip(eager, out):
        assert torch.equal(ei, gi) and torch.equal(ed, gd)
        assert (el is None and gl is None) or torch.equal(el, gl)


def test_bad_arguments_rejected_before_launch():
    import ctypes as C
    lib = _lib.load()
    e = torch.zeros((2, 256), device=DEV)
    g = torch.zeros((10, 256), device=DEV)
    for k in (0, 65):
        with pytest.raises(ValueError):
            ops.match_topk(e, g, k)
    with pytest.raises(ValueError, match="bad shape"):
        ops.match_topk(torch.zeros((2, 6), device=DEV), torch.zeros((10, 6), device=DEV), 2)    # D % 4 != 0 (the C entry rejects it)
    ws = torch.empty(lib.frmap_match_topk_workspace_bytes(2, 10, 256, 5), dtype=torch.uint8, device=DEV)
    idx = torch.empty((2, 5), dtype=torch.int32, device=DEV)
    dist = torch.empty((2, 5), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.frmap_match_topk(e.data_ptr(), g.data_ptr(), None, None, dist.data_ptr(), None, ws.data_ptr(), 2, 10, 256, 5, st) == -1
    assert "null pointer" in lib.frmap_last_error().decode()
    assert lib.frmap_match_topk(e.data_ptr(), g.data_ptr(), None, idx.data_ptr(), dist.data_ptr(), None, ws.data_ptr(), 2, 10, 256, 0, st) == -1
    assert "k=0" in lib.frmap_last_error().decode()
    assert lib.frmap_match_topk(e.data_ptr(), g.data_ptr(), None, idx.data_ptr(), dist.data_ptr(), None, ws.data_ptr(), 2, 10, 254, 5, st) == -1
    assert lib.frmap_match_topk_packed(e.data_ptr(), g.data_ptr(), None, None, None, idx.data_ptr(), dist.data_ptr(), None,
                                       ws.data_ptr(), 2, 10, 256, 65, st) == -1
    assert lib.frmap_match_topk_packed(e.data_ptr(), g.data_ptr(), g.data_ptr(), None, None, idx.data_ptr(), dist.data_ptr(), None,
                                       ws.data_ptr(), 2, 10, 256, 5, st) == -1
    assert "null pointer" in lib.frmap_last_error().decode()
    h = C.c_void_p()
    assert lib.frmap_model_create(C.byref(h), b"cnn", 36, 1) == 0
    assert lib.frmap_model_embed_and_search(h, e.data_ptr(), 0, 1, 224, 224, None, None, None, None, 0, 5, 0, idx.data_ptr(),
                                            dist.data_ptr(), None, None, ws.data_ptr(), st) == -1     # not finalized
    lib.frmap_model_destroy(h)


_CHILD = r'''
import ctypes as C, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import cabi_model_client as cc
vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
lib = cc.bind()
lib.frmap_model_search_workspace_bytes.restype = sz
lib.frmap_model_search_workspace_bytes.argtypes = [vp, i32, i32, i32, i32, i32]
lib.frmap_model_embed_and_search.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
lib.frmap_match_topk_workspace_bytes.restype = sz
lib.frmap_match_topk_workspace_bytes.argtypes = [i32, i32, i32, i32]
lib.frmap_match_topk_packed.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
lib.frmap_match_topk.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
dev = torch.device("cuda:0"); torch.cuda.set_device(dev); st = torch.cuda.current_stream().cuda_stream
a = np.load(sys.argv[3])
model = str(a["model"])
h = vp()
cc.check(lib, lib.frmap_model_create(C.byref(h), model.encode(), 36, 1), "create")
sd = np.load(sys.argv[2])
for key in sd.files:
    t = np.ascontiguousarray(sd[key], dtype=np.float32)
    cc.check(lib, lib.frmap_model_load_tensor(h, key.encode(), t.ctypes.data_as(vp), t.size, 0), key)
cc.check(lib, lib.frmap_model_finalize(h, st), "finalize")
x = torch.from_numpy(a["x"]).to(dev); B, _, H, W = x.shape
out = {}
for gname in ("small", "large"):
    gal = torch.from_numpy(a[gname]).to(dev); G, D = gal.shape
    lab = torch.from_numpy(a[gname + "_labels"]).to(dev)
    pk = st_w = None
    if G >= 512:
        pk = torch.empty(lib.frmap_match_gallery_pack_bytes(G, D), dtype=torch.uint8, device=dev)
        st_w = torch.empty((G, 4), dtype=torch.float32, device=dev)
        cc.check(lib, lib.frmap_match_pack_gallery(gal.data_ptr(), pk.data_ptr(), st_w.data_ptr(), G, D, st), "pack")
    pkp, stp = (pk.data_ptr(), st_w.data_ptr()) if pk is not None else (None, None)
    ws = torch.empty(lib.frmap_model_match_workspace_bytes(h, B, H, W, G), dtype=torch.uint8, device=dev)
    i1 = torch.empty(B, dtype=torch.int32, device=dev); d1 = torch.empty(B, dtype=torch.float32, device=dev)
    ids = torch.empty(B, dtype=torch.int32, device=dev)
    cc.check(lib, lib.frmap_model_embed_and_match(h, x.data_ptr(), 0, B, H, W, gal.data_ptr(), pkp, stp, G, 1.0, 1, i1.data_ptr(),
                                                  d1.data_ptr(), ids.data_ptr(), None, None, ws.data_ptr(), st), "match")
    for k, labels in ((1, None), (16, None), (16, lab)):
        ws2 = torch.empty(lib.frmap_model_search_workspace_bytes(h, B, H, W, G, k), dtype=torch.uint8, device=dev)
        ik = torch.empty((B, k), dtype=torch.int32, device=dev); dk = torch.empty((B, k), dtype=torch.float32, device=dev)
        lk = torch.empty((B, k), dtype=torch.int32, device=dev); emb = torch.empty((B, D), dtype=torch.float32, device=dev)
        lp = labels.data_ptr() if labels is not None else None
        cc.check(lib, lib.frmap_model_embed_and_search(h, x.data_ptr(), 0, B, H, W, gal.data_ptr(), pkp, stp, lp, G, k, 1,
                                                       ik.data_ptr(), dk.data_ptr(), lk.data_ptr(), emb.data_ptr(), ws2.data_ptr(), st), "search")
        # the same search on the handle's own embeddings
        ws3 = torch.empty(lib.frmap_match_topk_workspace_bytes(B, G, D, k), dtype=torch.uint8, device=dev)
        ir = torch.empty((B, k), dtype=torch.int32, device=dev); dr = torch.empty((B, k), dtype=torch.float32, device=dev)
        lr = torch.empty((B, k), dtype=torch.int32, device=dev)
        if pk is not None:
            cc.check(lib, lib.frmap_match_topk_packed(emb.data_ptr(), gal.data_ptr(), pkp, stp, lp, ir.data_ptr(), dr.data_ptr(),
                                                      lr.data_ptr(), ws3.data_ptr(), B, G, D, k, st), "topk_packed")
        else:
            cc.check(lib, lib.frmap_match_topk(emb.data_ptr(), gal.data_ptr(), lp, ir.data_ptr(), dr.data_ptr(), lr.data_ptr(),
                                               ws3.data_ptr(), B, G, D, k, st), "topk")
        torch.cuda.synchronize()
        tag = f"{gname}_k{k}_{'id' if labels is not None else 'entry'}"
        out.update({tag + "_idx": ik.cpu().numpy(), tag + "_dist": dk.cpu().numpy(), tag + "_lab": lk.cpu().numpy(),
                    tag + "_ridx": ir.cpu().numpy(), tag + "_rdist": dr.cpu().numpy(), tag + "_rlab": lr.cpu().numpy()})
    out[gname + "_m_idx"] = i1.cpu().numpy(); out[gname + "_m_dist"] = d1.cpu().numpy()
lib.frmap_model_destroy(h)
assert not any(m == "frmap_amd" or m.startswith("frmap_amd.") for m in sys.modules)
np.savez(sys.argv[4], **out)
'''


@pytest.mark.parametrize("mt", ["cnn", "arcface"])
def test_model_handle_embed_and_search(mt, tmp_path, calibrated_sd):
    from oracle import weights
    sd = calibrated_sd(mt)
    x = weights.golden_inputs(mt)
    B = x.shape[0]
    np.savez(tmp_path / "sd.npz", **{k: v.numpy() for k, v in sd.items() if v.dtype.is_floating_point})
    small = synth.unit_rows(1101, 36, 512, "tk_small").numpy()
    large = synth.unit_rows(1102, 900, 512, "tk_large").numpy()
    np.savez(tmp_path / "a.npz", model=np.array(mt), x=x.numpy(), small=small, large=large,
             small_labels=(np.arange(36) // 2).astype(np.int32), large_labels=(np.arange(900) % 300).astype(np.int32))
    (tmp_path / "child.py").write_text(_CHILD)
    r = subprocess.run([sys.executable, str(tmp_path / "child.py"), os.path.join(ROOT, "examples"), str(tmp_path / "sd.npz"),
                        str(tmp_path / "a.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    o = np.load(tmp_path / "out.npz")
    for gname in ("small", "large"):
        t = f"{gname}_k1_entry"
        assert np.array_equal(o[t + "_idx"][:, 0], o[gname + "_m_idx"]) and np.array_equal(o[t + "_dist"][:, 0], o[gname + "_m_dist"])
        assert (o[t + "_lab"] == -1).all()
        for t in (f"{gname}_k16_entry", f"{gname}_k16_id"):
            for f in ("idx", "dist", "lab"):
                assert np.array_equal(o[f"{t}_{f}"], o[f"{t}_r{f}"]), (t, f)
        assert (o[f"{gname}_k16_entry_idx"][:, 0] == o[gname + "_m_idx"]).all()
