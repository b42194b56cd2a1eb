// Which conv kernel runs a layer, and in which instantiation: the one place that decides.  Plain host C++ (no HIP): the
// launchers in conv_igemm.hip / conv_pp.hip turn a ConvPlan into a launch, the public layout / form / supported queries and
// the trace labels of model_api.cpp read the same plan, and tools/conv_plan_check.cpp runs the planner as a program of its own.
//
// THE ORDER (conv_plan).  The first row whose gate holds and whose candidate takes the layer wins; `dbg` is FRMAP_CONV_DEBUG,
// "pp on" the hook's enable when set, else FRMAP_CONV_PP (and the family's own switch and minimum Cin).
//
//   layer            | gate                               | candidate         | kernel
//   -----------------+------------------------------------+-------------------+------------------------------------------------
//   fused shortcut   | always, first                      | plan_fast         | must take it, else the call is an error
//   1x1              | dbg == 0 and Cin >= 128            | plan_pp_1x1       | conv1x1_pp_kernel<MI 7, WM, KS>
//   1x1              | dbg == 0 and Cin >= 128            | plan_1x1          | conv1x1_kernel<CKS> (stage = CKS chunks)
//   1x1              | else                               | plan_generic      | conv_igemm_kernel<256, 1, 1>
//   3x3 stride 2     | dbg == 0                           | plan_pp_s2        | conv3x3s2_pp_kernel<MI 7, WM, NHP>
//   3x3 stride 2     | dbg == 0 and even Hi               | plan_s2           | conv3x3s2_fast_kernel, else conv3x3s2_split_kernel
//   3x3 stride 1     | dbg == 0                           | plan_pp_3x3       | conv3x3_pp_kernel<MI 7, WM, NHP, KS, DS, IM, -, RI>
//   3x3              | always                             | plan_generic      | must fit ("rows too wide for LDS"), else an error
//   3x3 stride 1     | dbg == 0, no shortcut              | plan_wave         | conv3x3_c64_wave_kernel<NCH 2>
//   3x3 stride 1     | (shortcut: certain by row one)     | plan_fast         | conv3x3_fast_kernel<DS>
//   3x3              | else                               | plan_generic      | conv_igemm_kernel<BM, 3, stride>
//   -----------------+------------------------------------+-------------------+------------------------------------------------
//   3x3 + 2x2 pool   | Cin >= FRMAP_PP_POOL_MIN_CIN       | plan_pp_pool      | conv3x3_pp_kernel<.., PL>           (form 3)
//   3x3 + 2x2 pool   | always                             | plan_wave         | conv3x3_c64_wave_kernel<NCH, POOL>  (form 2)
//   3x3 + 2x2 pool   | always                             | plan_generic      | conv_igemm_kernel<BM, 3, 1, POOL>   (form 1)
//
// Two oddities are part of the order and stay: the generic fit is demanded in front of the wave kernel, which does not need it,
// and the Cin >= 128 gate sits in front of plan_pp_1x1, so frmap_conv1x1_pp_layout answers for narrower layers that
// frmap_conv_igemm never sends there.
#pragma once
#include <stdint.h>

// Every knob of the planners: environment values (read once, on first use of conv_tuning()) and the run-time hooks
// (frmap_conv_pp_tuning / _ri / _pitch / _ds / _im and frmap_conv_wave_start write here; -1 = not set, the environment or the heuristic decides).
struct ConvTuning {
  int debug;            // FRMAP_CONV_DEBUG (0): timing ablations of conv_igemm_kernel; any value keeps every other kernel out
  int s2fast;           // FRMAP_CONV_S2FAST (1)
  int wres;             // FRMAP_CONV_WRES (1): the weights-resident wave kernel for Cin = 64
  int dsfuse;           // FRMAP_CONV_DSFUSE (1)
  int ds_unfuse_small;  // FRMAP_DS_UNFUSE_SMALL (0): measured a wash end to end (eager +0.2 %, graph replay -3 %)
  int pool_wave;        // FRMAP_POOL_WAVE (1)
  int pool_min_cin;     // FRMAP_PP_POOL_MIN_CIN (128)
  int pp;               // FRMAP_CONV_PP (1)
  int pp_s2, pp_pool, pp_1x1;   // FRMAP_CONV_PP_S2 / _POOL / _1X1 (1)
  int pp_ds;            // FRMAP_CONV_PP_DS (1): fused 64.8 / 52.9 us at 28x28 / 14x14 (256 faces), first generation 72.4 / 68.4
  int min_tiles;        // FRMAP_PP_MIN_TILES (200): fewer tiles leave CUs idle, the first generation's smaller tiles win
  int min_cin;          // FRMAP_PP_MIN_CIN (128): Cin = 64 layers keep the wave kernel
  int s2_min_cin;       // FRMAP_PP_S2_MIN_CIN (64)
  int tile_px, bn;      // FRMAP_PP_TILE_PX, FRMAP_PP_BN (0 = heuristic; 3x3 stride 1 only)
  int fill;             // FRMAP_PP_FILL (1): conv_fill enlarges the image-aligned tiles towards the layout's capacity; 0 = off;
                        // A/B: a mask from 2 up fills 2 = 448 x 128 plain, 4 = with the shortcut, 8 = split-K, 16 = stride 2 only
  int pitch;            // FRMAP_PP_PITCH (0): conflict-free halo pitch
  int ri;               // FRMAP_PP_RI (0): fragment reads interleaved with the MFMAs
  int im;               // FRMAP_PP_IM (0): measured 4-6 % slower than issuing the DMA in the LOAD segments
  int wstart;           // FRMAP_WAVE_START (1): conv3x3_c64_wave_kernel issues its first tile's halo loads and every piece of the
                        // weight slab at once (0: the slab piece by piece, then the halo; A/B and tests)
  int h_on, h_px, h_bn, h_ks, h_ds, h_pitch, h_im, h_ri, h_wstart;   // hooks

  void set_tuning(int enable, int px, int bn_) {   // frmap_conv_pp_tuning; bn 1282 = the 128-channel tile with split-K
    h_on = enable;
    h_px = px;
    h_bn = bn_ == 1282 ? 128 : bn_;
    h_ks = bn_ == 1282 ? 2 : (bn_ == 128 || bn_ == 256 ? 1 : -1);
  }
  bool forced() const { return h_on >= 0; }
  bool pp_enabled(int family_on, int cin, int cin_min) const { return h_on >= 0 ? h_on != 0 : (pp && family_on && cin >= cin_min); }
  static int pick(int hook, int env) { return hook >= 0 ? hook : env; }
};
ConvTuning& conv_tuning();

enum ConvFuse { FUSE_NONE = 0, FUSE_RESIDUAL, FUSE_SHORTCUT, FUSE_POOL2 };
struct ConvLayer {
  int B, Hi, Wi, Cin, Cout, K, stride, pad;
  int fuse;                             // ConvFuse
  int ds_Hi, ds_Wi, ds_Cin, ds_stride;  // FUSE_SHORTCUT: the 1x1 projection's input map and stride
  int Ho() const { return (Hi + 2 * pad - K) / stride + 1; }
  int Wo() const { return (Wi + 2 * pad - K) / stride + 1; }
};

enum ConvKernel {
  CK_NONE = 0,   // not taken (ConvPlan::error says why where the cascade makes that an error)
  CK_IGEMM,      // conv_igemm_kernel<BM, KS, SWZ, POOL>
  CK_1X1,        // conv1x1_kernel<CKS>
  CK_WAVE,       // conv3x3_c64_wave_kernel<NCH, POOL>
  CK_FAST,       // conv3x3_fast_kernel<DS>
  CK_S2_SPLIT,   // conv3x3s2_split_kernel
  CK_S2_FAST,    // conv3x3s2_fast_kernel
  CK_PP,         // conv3x3_pp_kernel<MI, WM, NHP, KS, DS, IM, PL, RI>
  CK_PP_S2,      // conv3x3s2_pp_kernel<MI, WM, NHP>
  CK_PP_1X1,     // conv1x1_pp_kernel<MI, WM, KS>
};
struct ConvPlan {
  int kernel;                      // ConvKernel
  int BM, KS, SWZ, CKS, NCH;       // first generation (KS: taps per side there, split-K groups in the second generation)
  int MI, WM, NHP;                 // second generation
  bool DS, IM, PL, RI, POOL;
  bool EARLY;                      // wave kernel: ConvTuning::wstart
  int tile_px, mtiles, ntiles;     // second generation: grid = mtiles * ntiles
  int nblocks;                     // the grid, every family
  int halo_bytes, Wp, lds_bytes, ksplit;
  int wg_per_cu;                   // workgroups per CU the plan counts on (2: lds_bytes <= 80 KB)
  int layout;                      // what the family's public query answers (layout 1-3, pooled form 1-3)
  const char* label;               // trace label, "%s" = data type
  char error[112];
  bool taken() const { return kernel != CK_NONE; }
};

// candidates: the plan, or one with kernel == CK_NONE.  Pure: layer, tuning, CU count and the batch-invariant flag in, plan out.
ConvPlan plan_pp_3x3(const ConvLayer& L, const ConvTuning& t, bool inv);   // plain, residual or fused shortcut
ConvPlan plan_pp_s2(const ConvLayer& L, const ConvTuning& t, bool inv);
ConvPlan plan_pp_pool(const ConvLayer& L, const ConvTuning& t, bool inv);
ConvPlan plan_pp_1x1(const ConvLayer& L, const ConvTuning& t, int cus, bool inv);
ConvPlan plan_wave(const ConvLayer& L, const ConvTuning& t, int cus);      // plain / residual (Cin 64) or pooled (Cin 32 / 64)
ConvPlan plan_fast(const ConvLayer& L, const ConvTuning& t);               // register prefetch, with or without shortcut
ConvPlan plan_s2(const ConvLayer& L, const ConvTuning& t);                 // row-parity split staging: fast or split
ConvPlan plan_1x1(const ConvLayer& L, int ksplit);                         // ksplit is clamped to the stage count
ConvPlan plan_generic(const ConvLayer& L);                                 // 1x1, 3x3 or pooled 3x3; error set when rows do not fit

// the cascade of the table above; a layer must be one the entry points accept (K, stride, pad, Cin % 32, Cout % 64, sizes)
ConvPlan conv_plan(const ConvLayer& L, const ConvTuning& t, int cus, bool inv);

// THE FILL STEP.  conv_plan sizes a second-generation tile as whole images, or as a divisor of the image height (pp_tile_px):
// 392 of 448 pixels on 28x28 maps, 196 of 224 on 14x14 and 7x7 maps, while every wave still issues its full 7 x 4 MFMAs per
// k-step, the rest on clamped duplicate pixels (12.5 % of them).  The kernels take tiles that straddle images, so conv_fill
// enlarges the tile of a plan conv_plan has TAKEN (kernel, layout, split-K and every tile-count gate stay as decided on the
// image-aligned tile: the public layout queries answer as before) to the largest whole-row size <= the layout's capacity whose
// halo (pp_max_rows at the new size) still fits an instantiation that exists and 160 KB of LDS, and recomputes mtiles, nblocks,
// halo_bytes, NHP and lds_bytes.  Output elements keep their k order: the results are bit-identical.  Left as they are: the
// pooled form (its slices are whole row pairs), the 1x1 / match plans, a tile forced by FRMAP_PP_TILE_PX or the tuning hook, a
// plan that no larger size fits, the 224 px x 256 ch layouts (measured no faster filled: DESIGN.md), and everything when
// FRMAP_PP_FILL=0.  The launchers plan with conv_plan_launch.
ConvPlan conv_fill(const ConvLayer& L, const ConvPlan& q, const ConvTuning& t, bool inv);
inline ConvPlan conv_plan_launch(const ConvLayer& L, const ConvTuning& t, int cus, bool inv) { return conv_fill(L, conv_plan(L, t, cus, inv), t, inv); }

// THE KEY.  Every instantiation the launchers can dispatch has one canonical name, without the data type: the kernel and the
// template arguments the plan decides, flags by name where they are set - "conv_igemm_kernel<128,3,2>",
// "conv3x3_pp_kernel<7,2,5,1,DS>" (MI, WM, NHP, KS, then one of DS / IM / PL / RI), "conv3x3_c64_wave_kernel<1,POOL,EARLY>",
// "conv3x3s2_split_kernel<>".  The list of the keys is the table KEY_ROWS of conv_plan.cpp: a key beside the plan fields that
// select it.  The launchers' tables (conv_igemm.hip: CONV_KERNELS, conv_pp.hip: PP_KERNELS) hold the same keys beside the
// bf16 and fp16 function pointers and dispatch through them, so a name and a pointer cannot drift apart unseen:
// frmap_conv_plan_selfcheck walks the list.  (The match GEMM's modes are not conv layers and have no key.)
int conv_plan_key_index(const ConvPlan& q);                 // index into conv_plan_keys(), -1 = not taken / no such instantiation
const char* conv_plan_key(const ConvPlan& q);               // the key, "" = not taken / no such instantiation
int conv_plan_key(const ConvPlan& q, char* buf, int n);     // the same copied into buf (always terminated); returns its length
const char* const* conv_plan_keys(int* count);              // every key that exists
bool conv_plan_from_key(const char* key, ConvPlan* q);      // the plan fields that select `key` (nothing else set); false = no such key

// 1 = frmap_conv_igemm_ds takes the layer fused (and fusing is not switched off)
int conv_ds_supported(const ConvLayer& L, const ConvTuning& t, bool inv);

// frmap_linear_mfma: K slices of the split-K form (1 = none).  Batch-invariant: that of a single row tile for every M, so the
// fp32 summation order does not depend on the batch.
int linear_ksplit(int M, int K, int N, bool inv);
// the match GEMM (frmap_match_gemm_*, conv_pp.hip): 224 probes x 256 gallery rows per tile, or 448 x 128 when that fills the CUs better
ConvPlan match_gemm_plan(int P, int Gpad);

// most halo rows any tile touches (memoised); extra = 3 for stride 1, 2 for the half-resolution maps of stride 2
int pp_max_rows(long long M, int tile_px, int howo, int wo, int hp, int extra, bool inv);
