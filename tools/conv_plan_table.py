"""The conv planner's answers over a grid of shapes, through the public queries of the loaded library (no GPU needed).

    python tools/conv_plan_table.py --write tests/golden/conv_plan_parent.npz   # FRMAP_LIB=<.so> selects another build
    python tools/conv_plan_table.py --compare tests/golden/conv_plan_parent.npz

Ten answers per shape (COLUMNS): the five `*_layout` queries (1x1 at stride 1 and 2), `pool2_form`, `pool2_supported`,
`ds_supported` and `ds_layout` for a shortcut from a 2H x 2W map of max(32, Cin / 2) channels at stride 2, and the split-K
slices behind `frmap_linear_mfma_workspace_bytes`.  Two blocks: `main` (batch-invariant off / on x the tuning-hook settings of
tests/conv_cases.py x the shape grid) and `hooks` (default tuning, a smaller grid, under `frmap_conv_pp_pitch(1)` and
under `frmap_conv_pp_ds(0)`).  tests/test_conv_plan_cpu.py holds the library to the committed table of the commit before the
planner was gathered into csrc/conv_plan.cpp, and feeds the same rows to tools/conv_plan_check.cpp.
"""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COLUMNS = ("conv3x3_pp", "conv3x3s2_pp", "conv1x1_pp_s1", "conv1x1_pp_s2", "conv3x3_pp_pool", "pool2_form", "pool2_supported",
           "ds_supported", "conv3x3_pp_ds", "linear_ksplit")
TUNINGS = [(-1, -1, -1), (0, -1, -1), (1, -1, -1), (1, -1, 128), (1, -1, 256), (1, -1, 1282), (1, 37, 256)]
BATCHES = [1, 2, 8, 33, 256]
MAPS = [(1, 1), (2, 2), (3, 5), (4, 4), (7, 7), (8, 8), (10, 6), (13, 17), (14, 14), (16, 24), (20, 12), (28, 28), (56, 56), (61, 37),
        (112, 112), (150, 150)]
CINS = [32, 64, 96, 128, 160, 256, 512, 1024, 2048]
COUTS = [64, 128, 192, 256, 512, 640]
# the `hooks` block: default tuning, batch-invariant off
HOOK_BATCHES = [1, 33, 256]
HOOK_MAPS = [(3, 5), (7, 7), (10, 6), (14, 14), (20, 12), (28, 28), (56, 56), (61, 37), (112, 112)]
HOOK_CINS = [64, 128, 256, 512]
HOOK_COUTS = [128, 256, 512]
HOOKS = [("frmap_conv_pp_pitch", 1), ("frmap_conv_pp_ds", 0)]


def shapes(hooks=False):
    if hooks:
        return list(itertools.product(HOOK_BATCHES, HOOK_MAPS, HOOK_CINS, HOOK_COUTS))
    return list(itertools.product(BATCHES, MAPS, CINS, COUTS))


def shortcut_of(H, W, Cin):
    return 2 * H, 2 * W, max(32, Cin // 2), 2


def answers(lib, B, H, W, Ci, Co):
    ds = shortcut_of(H, W, Ci)
    return (lib.frmap_conv3x3_pp_layout(B, H, W, Ci, Co), lib.frmap_conv3x3s2_pp_layout(B, H, W, Ci, Co),
            lib.frmap_conv1x1_pp_layout(B, H, W, Ci, Co, 1), lib.frmap_conv1x1_pp_layout(B, H, W, Ci, Co, 2),
            lib.frmap_conv3x3_pp_pool_layout(B, H, W, Ci, Co), lib.frmap_conv_igemm_pool2_form(B, H, W, Ci, Co),
            lib.frmap_conv_igemm_pool2_supported(B, H, W, Ci, Co), lib.frmap_conv_igemm_ds_supported(B, H, W, Ci, Co, *ds),
            lib.frmap_conv3x3_pp_ds_layout(B, H, W, Ci, Co, *ds),
            min(255, lib.frmap_linear_mfma_workspace_bytes(B, Ci, Co) // (4 * B * Co)))


def reset_hooks(lib):
    lib.frmap_conv_pp_tuning(-1, -1, -1)
    lib.frmap_set_batch_invariant(-1)
    for name in ("frmap_conv_pp_pitch", "frmap_conv_pp_ds", "frmap_conv_pp_ri", "frmap_conv_pp_im"):
        getattr(lib, name)(-1)


def table(lib):
    """{"main": uint8 [2 * len(TUNINGS) * len(shapes()), 10], "hooks": uint8 [len(HOOKS) * len(shapes(True)), 10]}, rows in the
    order settings() lists them; the hooks are left reset whatever happens."""
    main, hooks = [], []
    try:
        reset_hooks(lib)
        for inv in (0, 1):
            lib.frmap_set_batch_invariant(inv)
            for tune in TUNINGS:
                lib.frmap_conv_pp_tuning(*tune)
                main.extend(answers(lib, B, H, W, Ci, Co) for B, (H, W), Ci, Co in shapes())
        reset_hooks(lib)
        for name, value in HOOKS:   # (the shortcut switch last: before the planner was gathered, a value it had once held stuck)
            getattr(lib, name)(value)
            hooks.extend(answers(lib, B, H, W, Ci, Co) for B, (H, W), Ci, Co in shapes(True))
            getattr(lib, name)(-1)
    finally:
        reset_hooks(lib)
    return {"main": np.array(main, dtype=np.uint8), "hooks": np.array(hooks, dtype=np.uint8)}


def settings():
    """The rows' settings, in table order: (block, batch_invariant, tuning, hook or None, B, H, W, Cin, Cout)."""
    out = []
    for inv in (0, 1):
        for tune in TUNINGS:
            out.extend(("main", inv, tune, None, B, H, W, Ci, Co) for B, (H, W), Ci, Co in shapes())
    for hook in HOOKS:
        out.extend(("hooks", 0, (-1, -1, -1), hook, B, H, W, Ci, Co) for B, (H, W), Ci, Co in shapes(True))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="NPZ")
    ap.add_argument("--compare", metavar="NPZ")
    args = ap.parse_args()
    from frmap_amd import _lib
    lib = _lib.load()
    t = table(lib)
    for block, a in t.items():
        print(block, a.shape, {c: sorted(set(a[:, i].tolist())) for i, c in enumerate(COLUMNS)})
    if args.write:
        np.savez_compressed(args.write, **t)
        print("wrote", args.write, os.path.getsize(args.write), "bytes, library", _lib.LIB_PATH)
    if args.compare:
        ref = np.load(args.compare)
        bad = {b: int((ref[b] != t[b]).any(axis=1).sum()) for b in t}
        print("rows that differ:", bad)
        rows = settings()
        off = 0
        for b in ("main", "hooks"):
            for i in np.nonzero((ref[b] != t[b]).any(axis=1))[0][:20]:
                print(rows[off + i], "file", ref[b][i].tolist(), "library", t[b][i].tolist())
            off += len(t[b])
        sys.exit(1 if any(bad.values()) else 0)


if __name__ == "__main__":
    main()
