// The planner's fill step (conv_fill, csrc/conv_plan.cpp) under the address and undefined-behaviour sanitizers, as a stand-alone
// host program: no Python, no GPU, no HIP; host-only work, not for a machine with a GPU.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Ifacerecognition-multiarchitecture-pipeline_amd/csrc tools/conv_fill_check.cpp -o /tmp/conv_fill_check && /tmp/conv_fill_check
//
// It prints one line per named case (tests/test_conv_fill_cpu.py asserts on them):
//   fill <name> B=.. kernel=.. layout=.. KS=.. WM=.. DS=.. PL=.. tile_px=.. mtiles=.. ntiles=.. NHP=.. halo=.. lds=.. base_tile_px=.. base_mtiles=.. base_NHP=..
// ("base_" = the plan of conv_plan, before the fill) and checks every filled plan, of the named cases and of a sweep of shapes
// under the default tuning and with the second generation forced on in each layout:
//   * the fill changes nothing but tile_px, mtiles, nblocks, halo_bytes, NHP and lds_bytes, and never shrinks a tile
//   * the tile is whole rows and <= the layout's capacity; mtiles covers M
//   * the halo of EVERY tile (walked one by one with the real M, as the kernels compute it) is <= halo_bytes <= NHP pieces
//   * NHP names an instantiation that exists; lds_bytes <= 160 KB
//   * with the switch at 0, with a forced tile size and for the pooled form the plan is conv_plan's
// A failed check is a line "FAIL ..." on stdout and exit status 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "conv_plan.cpp"

static int g_fail = 0;
static long g_plans = 0, g_filled = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      ++g_fail;                               \
      printf("FAIL %s: ", what);              \
      printf(__VA_ARGS__);                    \
      printf("  [%s]\n", #cond);              \
    }                                         \
  } while (0)

static const char* kernel_name(int k) { return k == CK_PP ? "conv3x3_pp_kernel" : (k == CK_PP_S2 ? "conv3x3s2_pp_kernel" : (k == CK_NONE ? "none" : "other")); }

static bool same_plan(const ConvPlan& a, const ConvPlan& b) {
  return a.kernel == b.kernel && a.BM == b.BM && a.KS == b.KS && a.SWZ == b.SWZ && a.CKS == b.CKS && a.NCH == b.NCH && a.MI == b.MI && a.WM == b.WM &&
         a.NHP == b.NHP && a.DS == b.DS && a.IM == b.IM && a.PL == b.PL && a.RI == b.RI && a.POOL == b.POOL && a.tile_px == b.tile_px &&
         a.mtiles == b.mtiles && a.ntiles == b.ntiles && a.nblocks == b.nblocks && a.halo_bytes == b.halo_bytes && a.Wp == b.Wp &&
         a.lds_bytes == b.lds_bytes && a.ksplit == b.ksplit && a.wg_per_cu == b.wg_per_cu && a.layout == b.layout && a.label == b.label;
}

// the halo rows of every tile, one by one, as conv3x3_pp_kernel / conv3x3s2_pp_kernel compute them
static long long worst_halo_bytes(long long M, int tile_px, int howo, int wo, int hp, int extra, int Wp) {
  long long worst = 0;
  for (long long m0 = 0; m0 < M; m0 += tile_px) {
    const long long mend = (m0 + tile_px < M ? m0 + tile_px : M) - 1;
    const long long n0 = m0 / howo, n1 = mend / howo;
    const long long rows = (n1 - n0) * hp + (mend - n1 * howo) / wo - (m0 - n0 * howo) / wo + extra;
    if (rows > worst) worst = rows;
  }
  return worst * Wp * 64;
}

// plans the layer, fills it, checks the filled plan; returns it
static ConvPlan filled(const char* what, const ConvLayer& L, const ConvTuning& t, int cus, bool inv, ConvPlan* base_out = nullptr) {
  const ConvPlan base = conv_plan(L, t, cus, inv);
  const ConvPlan q = conv_plan_launch(L, t, cus, inv);
  ++g_plans;
  if (base_out) *base_out = base;
  if (base.kernel != CK_PP && base.kernel != CK_PP_S2) {
    CHECK(same_plan(q, base), "%s is not a conv plan of the second generation, yet the fill changed it", kernel_name(base.kernel));
    return q;
  }
  ConvPlan r = q;   // nothing but the tile and what follows from it may differ
  r.tile_px = base.tile_px; r.mtiles = base.mtiles; r.nblocks = base.nblocks; r.halo_bytes = base.halo_bytes; r.NHP = base.NHP; r.lds_bytes = base.lds_bytes;
  CHECK(same_plan(r, base), "B=%d %dx%d Cin=%d Cout=%d: the fill changed more than the tile", L.B, L.Hi, L.Wi, L.Cin, L.Cout);
  CHECK(q.tile_px >= base.tile_px && q.mtiles <= base.mtiles, "tile %d -> %d, tiles %d -> %d", base.tile_px, q.tile_px, base.mtiles, q.mtiles);
  if (q.tile_px != base.tile_px) ++g_filled;
  const bool s2 = q.kernel == CK_PP_S2;
  const int Ho = s2 ? L.Hi / 2 : L.Hi, Wo = s2 ? L.Wi / 2 : L.Wi, Hp = s2 ? Ho + 1 : Ho + 2;
  const long long M = (long long)L.B * Ho * Wo;
  const int cap = (q.KS == 2 || q.WM == 2 ? 2 : 4) * 7 * 16;
  const bool tile_forced = (t.h_px > 0 && t.h_px <= cap) || (!s2 && t.tile_px > 0 && t.tile_px <= cap);
  CHECK(q.tile_px > 0 && q.tile_px <= cap && (tile_forced || q.tile_px % Wo == 0), "tile %d px, capacity %d, rows of %d", q.tile_px, cap, Wo);
  CHECK((long long)q.mtiles * q.tile_px >= M && (long long)(q.mtiles - 1) * q.tile_px < M && q.nblocks == q.mtiles * q.ntiles, "%d tiles of %d px over %lld",
        q.mtiles, q.tile_px, M);
  const long long halo = worst_halo_bytes(M, q.tile_px, Ho * Wo, Wo, Hp, s2 ? 2 : 3, q.Wp);
  const int piece = s2 ? 8192 : (8 / q.KS) * 1024;
  CHECK(halo <= q.halo_bytes && q.halo_bytes <= q.NHP * piece, "halo %lld, planned %d, %d pieces of %d", halo, q.halo_bytes, q.NHP, piece);
  if (s2) CHECK((q.NHP == 1 || q.NHP == 2 || (q.NHP == 4 && q.WM == 4)), "no conv3x3s2_pp_kernel<7, %d, %d>", q.WM, q.NHP);
  else if (q.KS == 2) CHECK((q.NHP == 4 || q.NHP == 6) && q.WM == 2 && !(q.RI && q.NHP == 6), "no split-K conv3x3_pp_kernel with NHP %d RI %d", q.NHP, q.RI);
  else CHECK((q.NHP == 3 || q.NHP == 5) && !(q.DS && q.WM == 4 && q.NHP == 3), "no conv3x3_pp_kernel<7, %d, %d> DS=%d", q.WM, q.NHP, q.DS);
  if (q.DS) CHECK(q.NHP * 8192 >= ((q.WM * 7 + 7) / 8) * 8192, "halo buffers of %d KB do not hold a gather image", q.NHP * 8);
  CHECK(q.lds_bytes > 0 && q.lds_bytes <= 160 * 1024, "lds_bytes %d", q.lds_bytes);
  return q;
}

static void show(const char* name, const ConvLayer& L, const ConvTuning& t, bool inv = false) {
  ConvPlan base;
  const ConvPlan q = filled(name, L, t, 256, inv, &base);
  printf("fill %s B=%d kernel=%s layout=%d KS=%d WM=%d DS=%d PL=%d tile_px=%d mtiles=%d ntiles=%d NHP=%d halo=%d lds=%d base_tile_px=%d base_mtiles=%d base_NHP=%d\n",
         name, L.B, kernel_name(q.kernel), q.layout, q.KS, q.WM, q.DS, q.PL, q.tile_px, q.mtiles, q.ntiles, q.NHP, q.halo_bytes, q.lds_bytes, base.tile_px,
         base.mtiles, base.NHP);
}

static ConvLayer conv(int B, int H, int W, int Ci, int Co, int stride = 1, int fuse = FUSE_NONE) { return ConvLayer{B, H, W, Ci, Co, 3, stride, 1, fuse, 0, 0, 0, 0}; }
static ConvLayer shortcut(int B, int H, int W, int Ci, int Co, int dsC) { return ConvLayer{B, H, W, Ci, Co, 3, 1, 1, FUSE_SHORTCUT, 2 * H, 2 * W, dsC, 2}; }

int main() {
  const ConvTuning base = conv_tuning();   // environment defaults, hooks unset
  const char* what = "setup";
  CHECK(base.fill == 1, "FRMAP_PP_FILL defaults to 1, got %d", base.fill);

  // ---- the flagship's layers (ResNet-18, 112 x 112 faces) at the two batch sizes it runs
  for (int B : {128, 256}) {
    show("l2.plain", conv(B, 28, 28, 128, 128), base);
    show("l2.residual", conv(B, 28, 28, 128, 128, 1, FUSE_RESIDUAL), base);
    show("l2.shortcut", shortcut(B, 28, 28, 128, 128, 64), base);
    show("l2.stride2", conv(B, 56, 56, 64, 128, 2), base);
    show("l3.plain", conv(B, 14, 14, 256, 256), base);
    show("l3.residual", conv(B, 14, 14, 256, 256, 1, FUSE_RESIDUAL), base);
    show("l3.shortcut", shortcut(B, 14, 14, 256, 256, 128), base);
    show("l3.stride2", conv(B, 28, 28, 128, 256, 2), base);
    show("l4.plain", conv(B, 7, 7, 512, 512), base);
    show("l4.shortcut", shortcut(B, 7, 7, 512, 512, 256), base);
    show("l4.stride2", conv(B, 14, 14, 256, 512, 2), base);
  }
  // ---- the layouts forced on through the hook, at the small batches of tests/test_conv_fill_gpu.py
  {
    ConvTuning t = base;
    t.set_tuning(1, -1, 256);
    show("hook.224x256", conv(9, 14, 14, 128, 256, 1, FUSE_RESIDUAL), t);
    show("hook.shortcut14", shortcut(9, 14, 14, 256, 256, 128), t);
    show("hook.stride2", conv(9, 28, 28, 128, 256, 2), t);
    t.set_tuning(1, -1, 128);
    show("hook.448x128", conv(5, 28, 28, 128, 128, 1, FUSE_RESIDUAL), t);
    show("hook.shortcut28", shortcut(5, 28, 28, 128, 128, 64), t);
    t.set_tuning(1, -1, 1282);
    show("hook.splitk", conv(9, 14, 14, 256, 256), t);
  }
  // ---- left alone: the switch at 0, a forced tile size (hook and environment value), the pooled form
  {
    ConvTuning off = base, hook = base, env = base;
    off.fill = 0;
    hook.set_tuning(-1, 392, -1);
    env.tile_px = 392;
    const ConvLayer l2 = conv(256, 28, 28, 128, 128), l3k = conv(128, 14, 14, 256, 256), s2 = conv(256, 56, 56, 64, 128, 2);
    what = "left alone";
    for (const ConvLayer& L : {l2, l3k, s2, shortcut(256, 28, 28, 128, 128, 64)}) {
      CHECK(same_plan(conv_plan_launch(L, off, 256, false), conv_plan(L, off, 256, false)), "FRMAP_PP_FILL=0 changed a plan (%dx%d)", L.Hi, L.Wi);
      // (392 px is more than the 224-pixel split-K layout holds: pp_tile_px does not apply it there, so that tile is not a forced one)
      CHECK(same_plan(conv_plan_launch(L, hook, 256, false), conv_plan(L, hook, 256, false)) == (L.Hi != 14), "the hook: forced tile filled, or an unforced one not (%dx%d)", L.Hi, L.Wi);
      // FRMAP_PP_TILE_PX = 392 is applied to the stride-1 448-pixel layouts only (stride 2 does not read it, 224-pixel layouts hold less)
      const bool env_applies = L.stride == 1 && L.Hi == 28;
      CHECK(same_plan(conv_plan_launch(L, env, 256, false), conv_plan(L, env, 256, false)) == env_applies, "FRMAP_PP_TILE_PX: forced tile filled, or an unforced one not (%dx%d)", L.Hi, L.Wi);
      CHECK(!same_plan(conv_plan_launch(L, base, 256, false), conv_plan(L, base, 256, false)), "the default plan was not filled (%dx%d): the cases above prove nothing", L.Hi, L.Wi);
    }
    // the 224 px x 256 ch layouts keep their tile (measured no faster filled): plain, shortcut, stride 2
    for (const ConvLayer& L : {conv(256, 14, 14, 256, 256), shortcut(256, 14, 14, 256, 256, 128), conv(256, 28, 28, 128, 256, 2)}) {
      const ConvPlan p = conv_plan(L, base, 256, false);
      CHECK((p.kernel == CK_PP || p.kernel == CK_PP_S2) && p.layout == 1 && same_plan(conv_plan_launch(L, base, 256, false), p), "a 224 x 256 plan was filled (%dx%d)", L.Hi, L.Wi);
    }
    show("off.l2", l2, off);
    show("forced.l2", l2, hook);
    ConvLayer pool = conv(256, 28, 28, 128, 128, 1, FUSE_POOL2);
    const ConvPlan p = conv_plan(pool, base, 256, false);
    CHECK(p.kernel == CK_PP && p.PL, "the pooled case does not take the ping-pong form (%d)", p.kernel);
    CHECK(same_plan(conv_plan_launch(pool, base, 256, false), p), "the pooled form was filled");
    show("pooled", pool, base);
    what = "1x1";
    const ConvLayer p1 = ConvLayer{256, 14, 14, 256, 256, 1, 1, 0, FUSE_NONE, 0, 0, 0, 0};
    CHECK(same_plan(conv_plan_launch(p1, base, 256, false), conv_plan(p1, base, 256, false)), "a 1x1 plan was filled");
  }
  // ---- batch-invariant planning: one tile size per geometry, whatever the batch
  for (int B : {1, 9, 256}) {
    show("inv.l3", conv(B, 14, 14, 256, 256), base, true);
    show("inv.l2", conv(B, 28, 28, 128, 128), base, true);
    show("inv.l3s2", conv(B, 28, 28, 128, 256, 2), base, true);
  }
  // ---- a sweep: every filled plan within the limits, whatever the shape
  {
    const int maps[][2] = {{2, 2}, {3, 5}, {4, 4}, {7, 7}, {8, 8}, {10, 6}, {13, 17}, {14, 14}, {16, 24}, {20, 12}, {28, 28}, {56, 56}, {61, 37}, {112, 112}};
    const int tunes[][3] = {{-1, -1, -1}, {1, -1, -1}, {1, -1, 128}, {1, -1, 256}, {1, -1, 1282}};
    what = "sweep";
    for (int inv = 0; inv < 2; ++inv)
      for (const auto& tu : tunes)
        for (int ri = 0; ri < 2; ++ri)
          for (int B : {1, 2, 9, 33, 256})
            for (const auto& hw : maps)
              for (int Ci : {32, 64, 128, 256, 512})
                for (int Co : {128, 256, 512}) {
                  ConvTuning t = base;
                  t.set_tuning(tu[0], tu[1], tu[2]);
                  t.h_ri = ri;
                  filled(what, conv(B, hw[0], hw[1], Ci, Co, 1, FUSE_RESIDUAL), t, 256, inv != 0);
                  filled(what, conv(B, hw[0], hw[1], Ci, Co, 2), t, 256, inv != 0);
                  const ConvLayer ds = shortcut(B, hw[0], hw[1], Ci, Co, Ci / 2 > 32 ? Ci / 2 : 32);
                  if (conv_ds_supported(ds, t, inv != 0)) filled(what, ds, t, 256, inv != 0);
                }
  }
  printf("conv_fill_check: %ld plans, %ld filled, %d failed checks\n", g_plans, g_filled, g_fail);
  return g_fail ? 1 : 0;
}
