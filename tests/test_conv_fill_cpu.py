"""CPU: the planner's fill step (`conv_fill`, csrc/conv_plan.cpp) as a stand-alone program under the address / undefined-behaviour
sanitizers (tools/conv_fill_check.cpp: its own `main` over csrc/conv_plan.cpp, nothing else; built with g++ and run directly).

The program prints the launch plan of every case next to the plan before the fill and checks each filled plan itself (whole rows,
within the capacity, the halo of every tile within the NHP pieces of an instantiation that exists, LDS <= 160 KB, nothing changed
but the tile and what follows from it; the same over a sweep of 60,000 plans).  This file asserts on the printed plans: the
flagship's layers get the tile sizes, tile counts and NHP worked out in DESIGN.md, layer 4 and everything the fill must leave
alone keep the plan they had, batch-invariant planning picks one tile per geometry.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
LDS_MAX = 160 * 1024


def _gpu_present():
    import torch
    return torch.cuda.is_available()


pytestmark = [
    pytest.mark.skipif(_gpu_present(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU"),
    pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with"),
]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(name, B): {field: value}} of every `fill` line, from one build and one run of the program."""
    tmp = tmp_path_factory.mktemp("conv_fill")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp / "conv_fill_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc,
                            os.path.join(ROOT, "tools", "conv_fill_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("FRMAP_")}   # the cases are about the default environment
    run = subprocess.run([exe], input="", capture_output=True, text=True, env=env)
    fails = [ln for ln in run.stdout.splitlines() if ln.startswith("FAIL")]
    assert run.returncode == 0 and not fails and run.stderr == "", "\n".join(fails[:20]) + run.stderr[-2000:]
    last = run.stdout.splitlines()[-1]
    assert last.startswith("conv_fill_check: ") and last.endswith(" 0 failed checks"), last
    assert int(last.split()[1]) > 50000 and int(last.split()[3]) > 10000, last          # the sweep ran, and filled plans were in it
    out = {}
    for ln in run.stdout.splitlines():
        if not ln.startswith("fill "):
            continue
        words = ln.split()
        f = dict(w.split("=", 1) for w in words[2:])
        f = {k: (v if k == "kernel" else int(v)) for k, v in f.items()}
        assert (words[1], f["B"]) not in out, ln
        out[(words[1], f["B"])] = f
    return out


def _pieces(p):
    """bytes the plan's NHP halo pieces hold: 8 waves x 1 KB each (split-K: 4 waves per group), stride 2 as the shared layouts"""
    return p["NHP"] * (8 // p["KS"]) * 1024


# name -> B -> (kernel, layout, tile_px, mtiles x ntiles, NHP, tile before, NHP before): DESIGN.md, "Measured (tile fill)"
PP, S2 = "conv3x3_pp_kernel", "conv3x3s2_pp_kernel"
FLAGSHIP = {
    "l2.plain": {128: (PP, 2, 448, 224, 5, 392, 5), 256: (PP, 2, 448, 448, 5, 392, 5)},
    "l2.residual": {128: (PP, 2, 448, 224, 5, 392, 5), 256: (PP, 2, 448, 448, 5, 392, 5)},
    "l2.shortcut": {128: (PP, 2, 448, 224, 5, 392, 5), 256: (PP, 2, 448, 448, 5, 392, 5)},
    # layer 3 at 128 faces: split-K, 112 x 2 channel tiles.  At 256 faces it runs in the 224 x 256 layout, which the fill step
    # skips: measured no faster filled ("Measured (tile fill)": 55.5 -> 56.2 us plain, 64.4 -> 64.2 us with the shortcut)
    "l3.plain": {128: (PP, 3, 224, 224, 6, 196, 4), 256: (PP, 1, 196, 256, 3, 196, 3)},
    "l3.residual": {128: (PP, 3, 224, 224, 6, 196, 4), 256: (PP, 1, 196, 256, 3, 196, 3)},
    "l3.shortcut": {256: (PP, 1, 196, 256, 3, 196, 3)},                                       # (128 faces: too few tiles, first generation)
    "l4.plain": {128: (PP, 3, 196, 128, 6, 196, 6), 256: (PP, 3, 196, 256, 6, 196, 6)},       # a seventh halo piece does not exist
}


@pytest.mark.parametrize("name", sorted(FLAGSHIP))
def test_flagship_layers_get_the_worked_out_tiles(plans, name):
    for B, (kernel, layout, px, tiles, nhp, px0, nhp0) in FLAGSHIP[name].items():
        p = plans[(name, B)]
        got = (p["kernel"], p["layout"], p["tile_px"], p["mtiles"] * p["ntiles"], p["NHP"], p["base_tile_px"], p["base_NHP"])
        assert got == (kernel, layout, px, tiles, nhp, px0, nhp0), (name, B, p)


def test_first_generation_layers_stay_where_they_were(plans):
    for key in (("l3.shortcut", 128), ("l3.stride2", 128), ("l4.shortcut", 128), ("l4.shortcut", 256), ("l4.stride2", 128), ("l4.stride2", 256)):
        assert plans[key]["kernel"] == "other" and plans[key]["tile_px"] == 0, (key, plans[key])


def test_stride2_layers_take_the_largest_whole_row_tile_whose_halo_has_an_instantiation(plans):
    """56 -> 28 (448 x 128 layout): 16 rows need five 8 KB pieces, which no instantiation has; 15 rows (420 px) fit four.
    28 -> 14 with 256 output channels runs in the 224 x 256 layout, which the fill step skips (40.9 -> 41.1 us filled to 210 px)."""
    for B in (128, 256):
        p = plans[("l2.stride2", B)]
        assert (p["kernel"], p["tile_px"], p["NHP"], p["base_tile_px"], p["base_NHP"]) == (S2, 420, 4, 392, 4), p
    p = plans[("l3.stride2", 256)]
    assert (p["kernel"], p["layout"], p["tile_px"], p["NHP"], p["base_tile_px"], p["base_NHP"]) == (S2, 1, 196, 2, 196, 2), p


def test_every_printed_plan_is_within_the_limits(plans):
    rows = {"l2": 28, "l3": 14, "l4": 7, "hook.224x256": 14, "hook.shortcut14": 14, "hook.stride2": 14, "hook.448x128": 28,
            "hook.shortcut28": 28, "hook.splitk": 14, "off.l2": 28, "forced.l2": 28, "pooled": 28, "inv.l3": 14, "inv.l2": 28, "inv.l3s2": 14}
    seen = 0
    for (name, B), p in plans.items():
        if p["kernel"] == "other":
            continue
        w = rows[name] if name in rows else rows[name.split(".")[0]]      # width of an output row
        assert p["tile_px"] % w == 0, (name, B, p)
        assert p["halo"] <= _pieces(p), (name, B, p)
        assert 0 < p["lds"] <= LDS_MAX, (name, B, p)
        assert p["tile_px"] >= p["base_tile_px"] and p["mtiles"] <= p["base_mtiles"], (name, B, p)
        seen += 1
    assert seen >= 30, seen


def test_hook_cases_of_the_gpu_test_are_filled_but_for_the_224x256_layout(plans):
    want = {("hook.224x256", 9): (1, 196, 9, 196), ("hook.448x128", 5): (2, 448, 9, 392), ("hook.splitk", 9): (3, 224, 8, 196),
            ("hook.shortcut14", 9): (1, 196, 9, 196), ("hook.shortcut28", 5): (2, 448, 9, 392), ("hook.stride2", 9): (1, 196, 9, 196)}
    for key, (layout, px, mtiles, px0) in want.items():
        p = plans[key]
        assert (p["layout"], p["tile_px"], p["mtiles"], p["base_tile_px"]) == (layout, px, mtiles, px0), (key, p)
    assert plans[("hook.splitk", 9)]["KS"] == 2 and plans[("hook.splitk", 9)]["NHP"] == 6
    assert plans[("hook.shortcut14", 9)]["DS"] == 1 and plans[("hook.shortcut28", 5)]["DS"] == 1


def test_switch_off_forced_tile_and_pooled_form_keep_the_parents_plan(plans):
    """(the program itself compares the whole plans field by field; here: the tiles are the image-aligned ones)"""
    for key in (("off.l2", 256), ("forced.l2", 256)):
        p = plans[key]
        assert (p["tile_px"], p["mtiles"], p["NHP"], p["halo"]) == (392, 512, 5, 30 * 1024) and p["base_tile_px"] == 392, (key, p)
    p = plans[("pooled", 256)]
    assert p["PL"] == 1 and (p["tile_px"], p["mtiles"], p["NHP"]) == (p["base_tile_px"], p["base_mtiles"], p["base_NHP"]) == (448, 448, 5), p


@pytest.mark.parametrize("name,px", [("inv.l3", 196), ("inv.l2", 448), ("inv.l3s2", 196)])
def test_batch_invariant_planning_picks_one_tile_per_geometry(plans, name, px):
    got = {B: (plans[(name, B)]["tile_px"], plans[(name, B)]["NHP"], plans[(name, B)]["halo"], plans[(name, B)]["layout"]) for B in (1, 9, 256)}
    assert got[1] == got[9] == got[256] and got[1][0] == px, got
