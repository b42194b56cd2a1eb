// The conv planner (csrc/conv_plan.cpp) under the address and undefined-behaviour sanitizers, as a stand-alone host program: no
// Python, no GPU, no HIP; host-only work, not for a machine with a GPU.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Ifacerecognition-multiarchitecture-pipeline_amd/csrc tools/conv_plan_check.cpp -o /tmp/conv_plan_check && /tmp/conv_plan_check < rows.txt
//
// Input, whitespace separated, one shape per record (tests/test_conv_plan_cpu.py writes the sweep of tools/conv_plan_table.py):
//   cus inv enable tile_px bn pitch ds  B H W Cin Cout  a0 .. a9
// (compute units; batch-invariant flag; the three frmap_conv_pp_tuning arguments; the pitch and shortcut hooks; the shape; the
// library's ten answers in the column order of tools/conv_plan_table.py).  For every record it plans the layers the answers speak
// of - 3x3 stride 1 plain and with a residual, 3x3 stride 2, 1x1 at stride 1 and 2, the 3x3 with the table's projection shortcut,
// the pooled 3x3 - prints every plan in full ("plan <layer> <kernel> ..." or "none <layer> <error>") and checks it:
//   * lds_bytes <= 160 KB, <= 80 KB where the plan counts on two workgroups per CU; halo_bytes / 64 < 65536; grid > 0
//   * a shortcut plan exists exactly where ds_supported answers 1, a pooled plan exactly where pool2_form != 0, of the form's family
//   * the candidates' layouts, the forms and the split-K slices are the library's answers
// A failed check is a line "FAIL ..." on stdout and exit status 1.  Without input it checks three layers of its own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "conv_plan.cpp"

static const char* kernel_name(int k) {
  static const char* names[] = {"none", "conv_igemm_kernel", "conv1x1_kernel", "conv3x3_c64_wave_kernel", "conv3x3_fast_kernel",
                                "conv3x3s2_split_kernel", "conv3x3s2_fast_kernel", "conv3x3_pp_kernel", "conv3x3s2_pp_kernel", "conv1x1_pp_kernel"};
  return k >= 0 && k <= CK_PP_1X1 ? names[k] : "?";
}

static int g_fail = 0;
static long g_plans = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      ++g_fail;                               \
      printf("FAIL %s: ", what);              \
      printf(__VA_ARGS__);                    \
      printf("  [%s]\n", #cond);              \
    }                                         \
  } while (0)

static ConvPlan planned(const char* what, const ConvLayer& L, const ConvTuning& t, int cus, bool inv) {
  const ConvPlan q = conv_plan(L, t, cus, inv);
  ++g_plans;
  if (!q.taken()) {
    printf("none %s B=%d %dx%d Cin=%d Cout=%d: %s\n", what, L.B, L.Hi, L.Wi, L.Cin, L.Cout, q.error);
    return q;
  }
  printf("plan %s B=%d %dx%d Cin=%d Cout=%d: %s BM=%d KS=%d SWZ=%d CKS=%d NCH=%d MI=%d WM=%d NHP=%d DS=%d IM=%d PL=%d RI=%d POOL=%d "
         "tile_px=%d mtiles=%d ntiles=%d nblocks=%d halo=%d Wp=%d lds=%d ksplit=%d per_cu=%d layout=%d label=%s\n",
         what, L.B, L.Hi, L.Wi, L.Cin, L.Cout, kernel_name(q.kernel), q.BM, q.KS, q.SWZ, q.CKS, q.NCH, q.MI, q.WM, q.NHP, q.DS, q.IM, q.PL,
         q.RI, q.POOL, q.tile_px, q.mtiles, q.ntiles, q.nblocks, q.halo_bytes, q.Wp, q.lds_bytes, q.ksplit, q.wg_per_cu, q.layout, q.label);
  CHECK(q.lds_bytes > 0 && q.lds_bytes <= 160 * 1024, "lds_bytes %d", q.lds_bytes);
  CHECK(q.wg_per_cu == 1 || q.lds_bytes <= 80 * 1024, "lds_bytes %d with %d workgroups per CU", q.lds_bytes, q.wg_per_cu);
  CHECK(q.halo_bytes >= 0 && q.halo_bytes / 64 < 65536, "halo_bytes %d", q.halo_bytes);
  CHECK(q.nblocks > 0, "grid %d", q.nblocks);
  CHECK(q.kernel < CK_PP || (q.mtiles > 0 && q.ntiles > 0 && q.tile_px > 0), "tiles %d x %d of %d px", q.mtiles, q.ntiles, q.tile_px);
  CHECK(q.label && strstr(q.label, kernel_name(q.kernel)) == q.label, "label %s", q.label ? q.label : "(null)");
  return q;
}

static void record(int cus, bool inv, const ConvTuning& t, int B, int H, int W, int Ci, int Co, const int* a) {
  const char* what = "answers";
  const ConvLayer s1 = {B, H, W, Ci, Co, 3, 1, 1, FUSE_NONE, 0, 0, 0, 0};
  ConvLayer res = s1, s2 = s1, p1 = s1, p2 = s1, ds = s1, pool = s1;
  res.fuse = FUSE_RESIDUAL;
  s2.stride = 2;
  p1.K = 1; p1.pad = 0;
  p2 = p1; p2.stride = 2;
  ds.fuse = FUSE_SHORTCUT; ds.ds_Hi = 2 * H; ds.ds_Wi = 2 * W; ds.ds_Cin = Ci / 2 > 32 ? Ci / 2 : 32; ds.ds_stride = 2;
  pool.fuse = FUSE_POOL2;
  // the candidates behind the public queries
  CHECK(plan_pp_3x3(s1, t, inv).layout == a[0], "conv3x3_pp %d, library %d", plan_pp_3x3(s1, t, inv).layout, a[0]);
  CHECK(plan_pp_s2(s2, t, inv).layout == a[1], "conv3x3s2_pp %d, library %d", plan_pp_s2(s2, t, inv).layout, a[1]);
  CHECK(plan_pp_1x1(p1, t, cus, inv).layout == a[2], "conv1x1_pp stride 1 %d, library %d", plan_pp_1x1(p1, t, cus, inv).layout, a[2]);
  CHECK(plan_pp_1x1(p2, t, cus, inv).layout == a[3], "conv1x1_pp stride 2 %d, library %d", plan_pp_1x1(p2, t, cus, inv).layout, a[3]);
  CHECK(plan_pp_pool(pool, t, inv).taken() == (a[4] != 0), "conv3x3_pp_pool %d, library %d", plan_pp_pool(pool, t, inv).taken(), a[4]);
  CHECK(conv_ds_supported(ds, t, inv) == a[7], "ds_supported %d, library %d", conv_ds_supported(ds, t, inv), a[7]);
  CHECK(plan_pp_3x3(ds, t, inv).layout == a[8], "conv3x3_pp_ds %d, library %d", plan_pp_3x3(ds, t, inv).layout, a[8]);
  const int ks = linear_ksplit(B, Ci, Co, inv);
  CHECK((ks > 1 ? (ks < 255 ? ks : 255) : 0) == a[9], "linear_ksplit %d, library %d", ks, a[9]);
  // the cascade
  what = "3x3"; planned(what, s1, t, cus, inv);
  what = "3x3+res"; planned(what, res, t, cus, inv);
  what = "3x3s2"; planned(what, s2, t, cus, inv);
  what = "1x1"; planned(what, p1, t, cus, inv);
  what = "1x1s2"; planned(what, p2, t, cus, inv);
  what = "3x3+shortcut";
  if (a[7]) {
    const ConvPlan q = planned(what, ds, t, cus, inv);
    CHECK(q.taken() && q.DS && (q.kernel == CK_FAST || q.kernel == CK_PP), "ds_supported 1, plan %s DS=%d", kernel_name(q.kernel), q.DS);
    CHECK((q.kernel == CK_PP) == (a[8] != 0), "conv3x3_pp_ds %d, plan %s", a[8], kernel_name(q.kernel));
  } else {
    CHECK(!conv_plan(ds, t, cus, inv).taken() || !t.dsfuse, "ds_supported 0, yet a shortcut plan %s", kernel_name(conv_plan(ds, t, cus, inv).kernel));
  }
  what = "3x3+pool";
  const ConvPlan q = planned(what, pool, t, cus, inv);
  CHECK(q.taken() == (a[5] != 0) && q.layout == a[5], "pool2_form %d, plan %s layout %d", a[5], kernel_name(q.kernel), q.layout);
  if (q.taken()) {
    CHECK(q.kernel == (a[5] == 3 ? CK_PP : a[5] == 2 ? CK_WAVE : CK_IGEMM) && (a[5] == 3 ? q.PL : q.POOL), "pool2_form %d, plan %s PL=%d POOL=%d", a[5],
          kernel_name(q.kernel), q.PL, q.POOL);
  }
  CHECK(((q.layout >= 2) || (q.layout == 1 && Ci <= 96)) == (a[6] != 0), "pool2_supported %d, form %d", a[6], q.layout);
}

int main() {
  ConvTuning base = conv_tuning();   // environment defaults, hooks unset
  int v[22], n = 0;
  long records = 0;
  while (scanf("%d", &v[n]) == 1) {
    if (++n < 22) continue;
    n = 0;
    ConvTuning t = base;
    t.set_tuning(v[2], v[3], v[4]);
    t.h_pitch = v[5]; t.h_ds = v[6];
    record(v[0], v[1] != 0, t, v[7], v[8], v[9], v[10], v[11], v + 12);
    ++records;
  }
  if (n) { fprintf(stderr, "conv_plan_check: input ends inside a record\n"); return 2; }
  if (!records) {   // no input: three layers whose plans are known (ResNet-18 at 256 faces, 256 CUs)
    const char* what = "self";
    const ConvPlan a = planned(what, ConvLayer{256, 56, 56, 64, 64, 3, 1, 1, FUSE_RESIDUAL, 0, 0, 0, 0}, base, 256, false);
    CHECK(a.kernel == CK_WAVE && a.nblocks == 256 && a.lds_bytes == 2 * 9 * 4096 + 8 * 10240, "%s grid %d lds %d", kernel_name(a.kernel), a.nblocks, a.lds_bytes);
    const ConvPlan b = planned(what, ConvLayer{256, 14, 14, 256, 256, 3, 1, 1, FUSE_NONE, 0, 0, 0, 0}, base, 256, false);
    CHECK(b.kernel == CK_PP && b.layout == 1 && b.tile_px == 196 && b.mtiles == 256 && b.ntiles == 1, "%s layout %d tile %d", kernel_name(b.kernel), b.layout, b.tile_px);
    const ConvPlan c = planned(what, ConvLayer{1, 7, 10, 64, 128, 3, 2, 1, FUSE_NONE, 0, 0, 0, 0}, base, 256, false);
    CHECK(c.kernel == CK_IGEMM && c.SWZ == 2, "%s SWZ %d (odd height: the generic kernel)", kernel_name(c.kernel), c.SWZ);
  }
  printf("conv_plan_check: %ld records, %ld plans, %d failed checks\n", records, g_plans, g_fail);
  return g_fail ? 1 : 0;
}
