// The conv planner (conv_plan.h): plain host C++, no HIP.
#include "conv_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <map>
#include <mutex>

static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

ConvTuning& conv_tuning() {
  static ConvTuning t = [] {
    ConvTuning v{};
    v.debug = env_int("FRMAP_CONV_DEBUG", 0);
    v.s2fast = env_int("FRMAP_CONV_S2FAST", 1);
    v.wres = env_int("FRMAP_CONV_WRES", 1);
    v.dsfuse = env_int("FRMAP_CONV_DSFUSE", 1);
    v.ds_unfuse_small = env_int("FRMAP_DS_UNFUSE_SMALL", 0);
    v.pool_wave = env_int("FRMAP_POOL_WAVE", 1);
    v.pool_min_cin = env_int("FRMAP_PP_POOL_MIN_CIN", 128);
    v.pp = env_int("FRMAP_CONV_PP", 1);
    v.pp_s2 = env_int("FRMAP_CONV_PP_S2", 1);
    v.pp_pool = env_int("FRMAP_CONV_PP_POOL", 1);
    v.pp_1x1 = env_int("FRMAP_CONV_PP_1X1", 1);
    v.pp_ds = env_int("FRMAP_CONV_PP_DS", 1);
    v.min_tiles = env_int("FRMAP_PP_MIN_TILES", 200);
    v.min_cin = env_int("FRMAP_PP_MIN_CIN", 128);
    v.s2_min_cin = env_int("FRMAP_PP_S2_MIN_CIN", 64);
    v.tile_px = env_int("FRMAP_PP_TILE_PX", 0);
    v.fill = env_int("FRMAP_PP_FILL", 1);
    v.bn = env_int("FRMAP_PP_BN", 0);
    v.pitch = env_int("FRMAP_PP_PITCH", 0);
    v.ri = env_int("FRMAP_PP_RI", 0);
    v.im = env_int("FRMAP_PP_IM", 0);
    v.wstart = env_int("FRMAP_WAVE_START", 1);
    v.h_on = v.h_px = v.h_bn = v.h_ks = v.h_ds = v.h_pitch = v.h_im = v.h_ri = v.h_wstart = -1;
    return v;
  }();
  return t;
}

// ------------------------------------------------------------------------------------------------
// shared rules
// ------------------------------------------------------------------------------------------------
static const long long LDS_MAX = 160 * 1024, LDS_HALF = 80 * 1024;

static long long round1k(long long v) { return (v + 1023) & ~1023ll; }

// dynamic LDS of a plan: the one place that knows the kernels' LDS layouts
static int plan_lds(const ConvPlan& q) {
  int lds = 0, scratch = 4 * 16 * (4 * 64 + 16);   // epilogue transpose region (4 waves; 8 in the second generation)
  const int wb = (q.KS == 2 ? 2 : 8 / (q.WM ? q.WM : 8)) * 64 * 64;   // second generation: one weight slab
  const int xch = q.KS == 2 ? 4 * q.MI * 4 * 1024 : 0;                // split-K: the groups' exchange region
  switch (q.kernel) {
    case CK_IGEMM: case CK_FAST: lds = q.halo_bytes + q.KS * q.KS * 4096; break;
    case CK_S2_SPLIT: case CK_S2_FAST: lds = q.halo_bytes + 6 * 4096; break;
    case CK_1X1: lds = q.CKS * (256 * 64 + 4096); break;
    case CK_WAVE: lds = q.NCH * 9 * 4096 + 8 * (10 * 16 * 64); break;
    case CK_PP:   // halo images | slab ring (5 slabs in the RI form of the shared-buffer layouts) | shortcut gather images
      lds = q.KS * (2 * q.NHP * (8 / q.KS) * 1024 + (q.RI && q.KS == 1 ? 5 : 4) * wb) + (q.DS ? ((q.WM * q.MI + 7) / 8) * 8192 : 0);
      break;
    case CK_PP_S2: lds = 4 * q.NHP * 8192 + 4 * wb; break;
    case CK_PP_1X1: {
      const int cap = (q.KS == 2 ? 2 : q.WM) * q.MI * 16, gw = 8 / q.KS, ngp = (cap / 16 + gw - 1) / gw;
      lds = q.KS * (3 * ngp * gw * 1024 + 4 * wb);
      break;
    }
  }
  if (q.kernel >= CK_PP) scratch *= 2;
  if (lds < scratch) lds = scratch;
  if (q.kernel >= CK_PP && lds < xch) lds = xch;
  return lds;
}
static ConvPlan finish(ConvPlan q, const char* label) {
  q.label = label;
  if (q.kernel >= CK_PP) q.nblocks = q.mtiles * q.ntiles;
  if (!q.ksplit) q.ksplit = 1;
  if (!q.wg_per_cu) q.wg_per_cu = 1;
  q.lds_bytes = plan_lds(q);
  return q;
}

// first generation: most output rows / image crossings BM consecutive flattened pixels can touch
static int halo_rows_bound(int BM, int Ho, int Wo, int Hp, int stride, int KS) {
  const int rows = (BM + Wo - 2) / Wo + 1;
  const int cross = (BM + Ho * Wo - 2) / (Ho * Wo);
  const int cross_step = Hp - (Ho - 1) * stride;  // padded-row jump from last row of n to first of n+1
  const int x = cross < rows - 1 ? cross : rows - 1;
  int gdiff = (rows - 1 - x) * stride + x * (cross_step > stride ? cross_step : stride);
  return gdiff + KS;
}
static int pool_rows_bound(int BM, int Ho, int Wo) {
  const int nw = BM / 4, Wo2 = Wo / 2, Win = (Ho / 2) * Wo2;
  const int pairs = (nw + Wo2 - 2) / Wo2 + 1;      // window rows BM/4 consecutive windows can touch
  const int cross = (nw + Win - 2) / Win;          // image crossings (each adds the Hp - Ho = 2 padding rows)
  const int x = cross < pairs - 1 ? cross : pairs - 1;
  return 2 * pairs + 2 * x + 2;
}
// the register-prefetch kernels read whole images around a tile with 32-bit offsets
static bool prefetch_offsets_fit(int HoWo, long long H, long long W, long long C) { return (256 / HoWo + 3) * H * W * C * 2 < (1ll << 31); }

// second generation, evaluated exactly as the kernels do, over one period of the tile start positions.
// Batch-invariant planning: the bound of an unbounded batch (every phase a tile start can have against the image grid: howo
// full tiles), so that whether a layer takes these kernels, and with how many halo pieces, follows from the per-image geometry
// alone.  With the actual M a tile that spans several small images (5 x 5 maps: 8 per tile) needed fewer rows at B = 1 than at
// B = 8, and a 160 x 160 input's last stride-2 layer ran on this kernel for one face and on another for eight.
int pp_max_rows(long long M, int tile_px, int howo, int wo, int hp, int extra, bool inv) {
  if (inv) M = (long long)howo * tile_px;
  // (memoised: the planner runs on every launch, the scan is up to one image's worth of tile starts)
  static std::mutex mu;
  static std::map<std::array<long long, 6>, int> memo;
  const std::array<long long, 6> key = {M, tile_px, howo, wo, hp, extra};
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = memo.find(key);
    if (it != memo.end()) return it->second;
  }
  int best = 0;
  const long long mtiles = (M + tile_px - 1) / tile_px;
  const long long lim = mtiles < howo ? mtiles : howo;
  for (long long mt = 0; mt < lim; ++mt) {
    const long long m0 = mt * tile_px, mend = (m0 + tile_px < M ? m0 + tile_px : M) - 1;
    const long long n0 = m0 / howo, n1 = mend / howo;
    const int oy0 = (int)((m0 - n0 * howo) / wo), oy1 = (int)((mend - n1 * howo) / wo);
    const int rows = (int)(n1 - n0) * hp + oy1 - oy0 + extra;
    if (rows > best) best = rows;
  }
  {
    std::lock_guard<std::mutex> lock(mu);
    if (memo.size() > 4096) memo.clear();
    memo[key] = best;
  }
  return best;
}

// Pixels per tile: whole images when they fit (7x7: 4 per 224, 14x14: 1), else whole rows - a divisor of the image height when
// one is within 1/8 of the capacity (28 rows, capacity 16 rows: 14), so tiles do not straddle images.
static int pp_tile_px(int cap, int H, int W, int forced_env, int forced_hook) {
  int tile_px;
  if (H * W <= cap) tile_px = (cap / (H * W)) * H * W;
  else {
    int rows = cap / W;
    for (int r = rows; r * 8 >= rows * 7 && r >= 1; --r)
      if (H % r == 0) { rows = r; break; }
    tile_px = rows * W;
  }
  if (forced_env > 0 && forced_env <= cap) tile_px = forced_env;
  if (forced_hook > 0 && forced_hook <= cap) tile_px = forced_hook;
  return tile_px;
}
// channel tile: 256 when Cout allows it, unless forced (a forced 256 falls back to 128 where Cout % 256)
static int pp_bn(int Cout, int forced_env, int forced_hook) {
  int bn = Cout % 256 == 0 ? 256 : 128;
  if (forced_env == 128 || forced_env == 256) bn = (forced_env == 256 && Cout % 256) ? 128 : forced_env;
  if (forced_hook == 128 || forced_hook == 256) bn = (forced_hook == 256 && Cout % 256) ? 128 : forced_hook;
  return bn;
}
static bool pp_sizes_fit(long long M, long long in_elems) { return M < (1ll << 31) && in_elems * 2 < (1ll << 46); }

// The instantiations conv_pp.hip builds, by halo size.  Stride 1: pieces of (8 / ks) KB per wave, at most 5 in the shared-buffer
// layouts and 6 with split-K (0 = no fit); classes NHP 3 / 5, split-K 4 / 6.  The shortcut form's halo buffers also hold a gather
// image: the 448-pixel layout (bn = 128) needs the 40 KB buffers of NHP = 5 for it.
static int pp_halo_pieces(long long hbytes, int ks) {
  const int per = (8 / ks) * 1024;
  const int nhp = (int)((hbytes + per - 1) / per);
  return nhp <= (ks == 2 ? 6 : 5) ? nhp : 0;
}
static int pp_nhp_class(int nhp, int ks, int bn, bool has_ds) {
  if (has_ds) return bn == 256 && nhp <= 3 ? 3 : 5;
  return ks == 2 ? (nhp <= 4 ? 4 : 6) : (nhp <= 3 ? 3 : 5);
}
// Stride 2: four sub-position images of NHP x 8 KB; NHP in {1, 2, 4}, and 4 only with bn = 128 (4 x 32 KB images + 4 x 16 KB
// slabs would not fit).  0 = no fit.
static int pp_s2_nhp_class(long long hbytes, int bn) {
  const int need = (int)((hbytes + 8191) / 8192);
  const int nhp = need <= 1 ? 1 : (need <= 2 ? 2 : (need <= 4 ? 4 : 0));
  return nhp == 4 && bn == 256 ? 0 : nhp;
}

// ------------------------------------------------------------------------------------------------
// second generation (conv_pp.hip)
// ------------------------------------------------------------------------------------------------
ConvPlan plan_pp_3x3(const ConvLayer& L, const ConvTuning& t, bool inv) {
  constexpr int MI = 7;
  ConvPlan q{};
  const int B = L.B, Hi = L.Hi, Wi = L.Wi, Cin = L.Cin, Cout = L.Cout;
  const bool has_ds = L.fuse == FUSE_SHORTCUT;
  if (!t.pp_enabled(1, Cin, t.min_cin)) return q;   // (forced on by the hook: every Cin % 32 == 0)
  if (Cin % 32 || Cin > 1024 || Cout % 128) return q;
  const long long Mll = (long long)B * Hi * Wi;
  if (!pp_sizes_fit(Mll, Mll * Cin)) return q;
  const int Hp = Hi + 2;
  // LDS pitch of a halo row (pixels).  A 16-pixel MFMA fragment that wraps an output row continues Wp - Wi + 1 pixels
  // further on; with Wp = Wi (mod 8) that keeps the fragment's 16-byte slots on distinct banks (the swizzle repeats every 8
  // pixels).  Columns past Wi + 1 are just more zero padding for the DMA.  (A/B: FRMAP_PP_PITCH)
  int Wp = Wi + 2;
  if (ConvTuning::pick(t.h_pitch, t.pitch)) { while (Wp % 8 != Wi % 8) ++Wp; }
  if (has_ds) {
    if (L.ds_Cin <= 0 || L.ds_Cin % 32 || L.ds_stride < 1 || (L.ds_Hi - 1) / L.ds_stride + 1 != Hi ||
        (L.ds_Wi - 1) / L.ds_stride + 1 != Wi || (long long)B * L.ds_Hi * L.ds_Wi * L.ds_Cin * 2 >= (1ll << 46))
      return q;
    if (!ConvTuning::pick(t.h_ds, t.pp_ds) && !t.forced()) return q;
  }
  // A layout = (pixels a tile can hold, channel tile, split-K groups).  Returns the halo pieces (KB / waves) needed, 0 = no fit.
  auto layout = [&](int cap, int bn, int ks, int& tile_px, int& mtiles, int& ntiles, int& hbytes_out) -> int {
    if (Wi > cap || Cout % bn || (ks == 2 && (Cin / 32) % 2)) return 0;
    tile_px = pp_tile_px(cap, Hi, Wi, t.tile_px, t.h_px);
    mtiles = (int)((Mll + tile_px - 1) / tile_px);
    ntiles = Cout / bn;
    const long long hbytes = (long long)pp_max_rows(Mll, tile_px, Hi * Wi, Wi, Hp, 3, inv) * Wp * 64;
    if (hbytes / 64 >= 65536) return 0;
    hbytes_out = (int)hbytes;
    return pp_halo_pieces(hbytes, ks);
  };
  // candidates: 224 px x 256 ch; 448 px x 128 ch; split-K 224 px x 128 ch (twice the tiles of either)
  int tpx = 0, mtl = 0, ntl = 0, hby = 0, ks = 1, bn = pp_bn(Cout, t.bn, t.h_bn);
  int nhp = layout(bn == 256 ? 2 * MI * 16 : 4 * MI * 16, bn, 1, tpx, mtl, ntl, hby);
  // (batch-invariant: layout from the per-image geometry alone - no tile-count rules, no split-K)
  const bool want_ks2 = !has_ds && !inv && (t.h_ks == 2 || (t.h_ks < 0 && (!nhp || (long long)mtl * ntl < t.min_tiles)));
  if (want_ks2 && t.h_ks != 1) {
    int t2 = 0, m2 = 0, n2 = 0, h2 = 0;
    const int nhp2 = layout(2 * MI * 16, 128, 2, t2, m2, n2, h2);
    if (nhp2 && (t.h_ks == 2 || !nhp || (long long)m2 * n2 > (long long)mtl * ntl)) {
      nhp = nhp2; tpx = t2; mtl = m2; ntl = n2; hby = h2; ks = 2; bn = 128;
    }
  }
  if (!nhp) return q;
  if (!inv && !t.forced() && (long long)mtl * ntl < t.min_tiles / 2) return q;   // too few tiles even with split-K: the smaller first-generation tiles win
  if (!inv && has_ds && (long long)mtl * ntl < t.min_tiles && !t.forced()) return q;   // (no split-K form of the shortcut kernel)
  q.kernel = CK_PP; q.MI = MI; q.KS = ks; q.DS = has_ds;
  q.tile_px = tpx; q.mtiles = mtl; q.ntiles = ntl; q.Wp = Wp; q.halo_bytes = hby;
  q.layout = ks == 2 ? 3 : (bn == 256 ? 1 : 2);
  q.WM = bn == 256 || ks == 2 ? 2 : 4;
  q.NHP = pp_nhp_class(nhp, ks, bn, has_ds);
  if (has_ds) return finish(q, "conv3x3_pp_kernel<%s, DS>");   // pixel-split layouts only
  // RI form (plain layers): fragment reads under the MFMAs.  (The RI form of the split-K layout with 6 halo pieces needs 258
  // VGPRs: it would spill inside the DMA-counted loop, so that one layout keeps the burst-read form; csrc/build.sh rejects any
  // *_pp_kernel with scratch)
  q.RI = ConvTuning::pick(t.h_ri, t.ri) != 0 && !(ks == 2 && nhp > 4);
  q.IM = !q.RI && ConvTuning::pick(t.h_im, t.im) != 0;
  return finish(q, "conv3x3_pp_kernel<%s>");
}

// 3x3 stride-2 pad-1, even input sizes: space-to-depth addressing; the half-resolution maps carry a top / left border only
ConvPlan plan_pp_s2(const ConvLayer& L, const ConvTuning& t, bool inv) {
  constexpr int MI = 7;
  ConvPlan q{};
  const int B = L.B, Hi = L.Hi, Wi = L.Wi, Cin = L.Cin, Cout = L.Cout;
  if (!t.pp_enabled(t.pp_s2, Cin, t.s2_min_cin)) return q;
  if (Hi % 2 || Wi % 2 || Cin % 32 || Cin > 1024 || Cout % 128) return q;
  const int Ho = Hi / 2, Wo = Wi / 2;
  const long long Mll = (long long)B * Ho * Wo;
  if (!pp_sizes_fit(Mll, (long long)B * Hi * Wi * Cin) || (long long)Hi * Wi * Cin * 2 >= (1ll << 31)) return q;
  const int bn = pp_bn(Cout, 0, t.h_bn);
  const int cap = (bn == 256 ? 2 : 4) * MI * 16;
  if (Wo > cap) return q;
  const int tile_px = pp_tile_px(cap, Ho, Wo, 0, t.h_px);
  q.MI = MI; q.WM = bn == 256 ? 2 : 4; q.KS = 1;
  q.Wp = Wo + 1;
  q.tile_px = tile_px;
  q.mtiles = (int)((Mll + tile_px - 1) / tile_px);
  q.ntiles = Cout / bn;
  const long long hbytes = (long long)pp_max_rows(Mll, tile_px, Ho * Wo, Wo, Ho + 1, 2, inv) * q.Wp * 64;
  if (hbytes / 64 >= 65536) return q;
  q.halo_bytes = (int)hbytes;
  q.NHP = pp_s2_nhp_class(hbytes, bn);
  if (!q.NHP) return q;
  if (!inv && !t.forced() && (long long)q.mtiles * q.ntiles < t.min_tiles) return q;
  q.kernel = CK_PP_S2;
  q.layout = bn == 256 ? 1 : 2;
  return finish(q, "conv3x3s2_pp_kernel<%s>");
}

// conv3x3 s1 p1 + shift (+ReLU) + MaxPool2d(2, 2) (PL = true).  Takes maps whose row pairs tile a wave's 112-pixel slice
// (Wi in {2, 4, 8, 14, 28, 56}, even Hi), Cin % 32 == 0, Cout % 128 == 0; tiles are WM whole slices.
ConvPlan plan_pp_pool(const ConvLayer& L, const ConvTuning& t, bool inv) {
  ConvPlan q{};
  const int B = L.B, Hi = L.Hi, Wi = L.Wi, Cin = L.Cin, Cout = L.Cout;
  if (!t.pp_enabled(t.pp_pool, Cin, 0)) return q;
  if (Hi % 2 || Wi % 2 || 112 % (2 * Wi) || Cin % 32 || Cin > 1024 || Cout % 128) return q;
  const long long Mll = (long long)B * Hi * Wi;
  if (!pp_sizes_fit(Mll, Mll * Cin)) return q;
  q.Wp = Wi + 2;
  int bn = pp_bn(Cout, 0, t.h_bn), nhp = 0;
  for (int attempt = 0; attempt < 2 && !nhp; ++attempt) {
    const int tile_px = (bn == 256 ? 2 : 4) * 112;
    const long long hbytes = (long long)pp_max_rows(Mll, tile_px, Hi * Wi, Wi, Hi + 2, 3, inv) * q.Wp * 64;
    const int n = (int)((hbytes + 8191) / 8192);
    if (hbytes / 64 < 65536 && n <= 5) { nhp = n; q.tile_px = tile_px; q.halo_bytes = (int)hbytes; }
    else bn = bn == 256 ? 128 : 256;   // the other layout (a wider tile has fewer halo rows per pixel, a narrower one fewer rows)
    if (!nhp && Cout % bn) break;
  }
  if (!nhp) return q;
  q.kernel = CK_PP; q.PL = true; q.MI = 7; q.KS = 1;
  q.WM = bn == 256 ? 2 : 4; q.NHP = nhp <= 3 ? 3 : 5;
  q.mtiles = (int)((Mll + q.tile_px - 1) / q.tile_px); q.ntiles = Cout / bn;
  q.layout = 3;
  return finish(q, "conv3x3_pp_kernel<%s, PL>");
}

// 1x1 conv / Linear.  Layouts: 1 = 224 px x 256 ch, 2 = 448 px x 128 ch, 3 = split-K 224 px x 128 ch.  One workgroup per CU, so
// what counts is ROUNDS x time per tile: est = ceil(tiles / CUs) x (k-steps per group x 0.6 us + 7.5 us of prologue and epilogue);
// 280 tiles on 256 CUs are two rounds.  The first-generation kernel (small tiles, two workgroups per CU) is modelled at 470 TFLOP/s.
ConvPlan plan_pp_1x1(const ConvLayer& L, const ConvTuning& t, int cus, bool inv) {
  ConvPlan q{};
  const int B = L.B, Hi = L.Hi, Wi = L.Wi, Cin = L.Cin, Cout = L.Cout, stride = L.stride;
  if (!t.pp_enabled(t.pp_1x1, Cin, 0)) return q;
  if (inv && !t.forced()) return q;   // (its layout is a rounds x time estimate over the tile count: the first-generation kernel's is not)
  if (Cin % 32 || Cin > 16384 || Cout % 128 || stride < 1) return q;
  const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1, nchunks = Cin / 32;
  const long long Mll = (long long)B * Ho * Wo;
  if (!pp_sizes_fit(Mll, (long long)B * Hi * Wi * Cin)) return q;
  auto est_us = [&](int lay) -> double {
    if (lay == 1 && Cout % 256) return 1e30;
    if (lay == 3 && nchunks % 2) return 1e30;
    const int px = lay == 2 ? 448 : 224, bn = lay == 1 ? 256 : 128;
    const long long tiles = ((Mll + px - 1) / px) * (Cout / bn);
    const long long rounds = (tiles + cus - 1) / cus;
    return (double)rounds * ((lay == 3 ? nchunks / 2 : nchunks) * 0.6 + 7.5);
  };
  int layout = 0;
  double best = 1e30;
  for (int lay = 1; lay <= 3; ++lay) {
    if (t.h_bn == 256 && t.h_ks != 2 && lay != 1 && Cout % 256 == 0) continue;   // forced by the tuning hook
    if (t.h_bn == 128 && t.h_ks == 1 && lay != 2) continue;
    if (t.h_ks == 2 && lay != 3 && nchunks % 2 == 0) continue;
    const double e = est_us(lay);
    if (e < best) { best = e; layout = lay; }
  }
  if (!layout || best >= 1e30) return q;
  if (!t.forced()) {
    const double gen1_us = 2.0 * (double)Mll * Cin * Cout / 470e6;
    if (best > 0.9 * gen1_us || t.min_tiles < 0) return q;   // (a clear win only: AttentionNet's 640-channel q/k/v conv is 140 tiles - 29 us here, 19 there)
  }
  q.kernel = CK_PP_1X1; q.MI = 7; q.WM = layout == 2 ? 4 : 2; q.KS = layout == 3 ? 2 : 1;
  q.Wp = Wo;          // (output geometry: the kernel needs no padded map)
  q.tile_px = layout == 2 ? 448 : 224;
  q.mtiles = (int)((Mll + q.tile_px - 1) / q.tile_px);
  q.ntiles = Cout / (layout == 1 ? 256 : 128);
  q.layout = layout;
  return finish(q, "conv1x1_pp_kernel<%s>");
}

ConvPlan match_gemm_plan(int P, int Gpad) {
  const long long t1 = ((P + 223) / 224) * (long long)(Gpad / 256), t2 = ((P + 447) / 448) * (long long)(Gpad / 128);
  const long long r1 = (t1 + 255) / 256, r2 = (t2 + 255) / 256;   // rounds on 256 CUs (a tile costs the same in both layouts)
  const bool wide = r2 < r1 || (r2 == r1 && t2 > t1);             // same rounds: the layout that occupies more CUs
  ConvPlan q{};
  q.kernel = CK_PP_1X1; q.MI = 7; q.WM = wide ? 4 : 2; q.KS = 1;
  q.Wp = 1;
  q.tile_px = wide ? 448 : 224;
  q.mtiles = (P + q.tile_px - 1) / q.tile_px;
  q.ntiles = Gpad / (wide ? 128 : 256);
  q.layout = wide ? 2 : 1;
  return finish(q, "conv1x1_pp_kernel<F16, MATCH>");
}

// ------------------------------------------------------------------------------------------------
// first generation (conv_igemm.hip)
// ------------------------------------------------------------------------------------------------
// weights-resident wave-autonomous kernel: one 8-wave workgroup per CU (per channel tile), each wave walks 8x8 patches
ConvPlan plan_wave(const ConvLayer& L, const ConvTuning& t, int cus) {
  ConvPlan q{};
  const bool pool = L.fuse == FUSE_POOL2;
  if (L.K != 3 || L.stride != 1 || L.fuse == FUSE_SHORTCUT || L.Hi % 8 || L.Wi % 8) return q;
  if (pool ? !(t.pool_wave && (L.Cin == 32 || L.Cin == 64)) : !(t.wres && t.debug == 0 && L.Cin == 64)) return q;
  if ((long long)L.Hi * L.Wi * L.Cin * 2 >= (1ll << 31) || (long long)(pool ? 4 * (L.Wi / 2) : 8 * L.Wi) * L.Cout * 2 >= (1ll << 31)) return q;
  const int ntiles = L.Cout / 64, total = L.B * (L.Hi / 8) * (L.Wi / 8);
  int per = cus / ntiles;
  if (per < 1) per = 1;
  if (per > (total + 7) / 8) per = (total + 7) / 8;
  q.kernel = CK_WAVE; q.NCH = L.Cin / 32; q.POOL = pool; q.KS = 3;
  q.EARLY = ConvTuning::pick(t.h_wstart, t.wstart) != 0;
  q.nblocks = per * ntiles; q.ntiles = ntiles;
  q.Wp = L.Wi + 2;
  q.layout = pool ? 2 : 0;
  return finish(q, pool ? "conv3x3_c64_wave_kernel<%s, POOL>" : "conv3x3_c64_wave_kernel<%s>");
}

// register-prefetch persistent kernel: the whole halo of a 256-pixel tile is <= 10 pieces per thread, two workgroups per CU.
// With a shortcut its chunks ride in the main loop's stages: no more of them than main chunks, and a halo that holds a stage.
ConvPlan plan_fast(const ConvLayer& L, const ConvTuning& t) {
  ConvPlan q{};
  if (L.K != 3 || L.stride != 1 || L.pad != 1 || L.fuse == FUSE_POOL2 || t.debug != 0) return q;
  const int Hi = L.Hi, Wi = L.Wi, Wp = Wi + 2;
  const long long raw = (long long)halo_rows_bound(256, Hi, Wi, Hi + 2, 1, 3) * Wp * 64, hb = round1k(raw);
  if (raw + 9 * 4096 > LDS_MAX || hb / 16 > 10 * 256 || hb + 9 * 4096 > LDS_HALF || !prefetch_offsets_fit(Hi * Wi, Hi, Wi, L.Cin)) return q;
  if (L.fuse == FUSE_SHORTCUT) {
    if (L.ds_Cin <= 0 || L.ds_Cin % 32 || L.ds_Cin / 32 > L.Cin / 32 || L.ds_stride < 1) return q;
    if ((L.ds_Hi - 1) / L.ds_stride + 1 != Hi || (L.ds_Wi - 1) / L.ds_stride + 1 != Wi) return q;  // 1x1, pad 0: Ho = (H-1)/s + 1
    if (hb < 256 * 64 || !prefetch_offsets_fit(Hi * Wi, L.ds_Hi, L.ds_Wi, L.ds_Cin)) return q;
  }
  q.kernel = CK_FAST; q.BM = 256; q.KS = 3; q.SWZ = 1; q.DS = L.fuse == FUSE_SHORTCUT;
  q.halo_bytes = (int)hb; q.Wp = Wp; q.wg_per_cu = 2;
  q.ntiles = L.Cout / 64;
  q.nblocks = (int)(((long long)L.B * Hi * Wi + 255) / 256) * q.ntiles;
  return finish(q, q.DS ? "conv3x3_fast_kernel<%s, true>" : "conv3x3_fast_kernel<%s, false>");
}

// 3x3 stride 2, even input height: row-parity split staging, two workgroups per CU; the fast form prefetches in registers
ConvPlan plan_s2(const ConvLayer& L, const ConvTuning& t) {
  ConvPlan q{};
  if (L.K != 3 || L.stride != 2 || L.Hi % 2 || t.debug != 0) return q;
  const int Ho = L.Ho(), Wo = L.Wo(), Hp = L.Hi + 2, Wp = L.Wi + 2;
  const int rows = (256 + Wo - 2) / Wo + 1, cross = (256 + Ho * Wo - 2) / (Ho * Wo);
  const int x = cross < rows - 1 ? cross : rows - 1;
  const int step = Hp / 2 - (Ho - 1);
  const long long hbs = round1k((long long)((rows - 1 - x) + x * (step > 1 ? step : 1) + 2) * Wp * 64);
  if (hbs + 6 * 4096 > LDS_HALF || hbs / 64 >= 65536) return q;
  const bool fast = t.s2fast && hbs / 16 <= 12 * 256 && prefetch_offsets_fit(Ho * Wo, L.Hi, L.Wi, L.Cin);
  q.kernel = fast ? CK_S2_FAST : CK_S2_SPLIT; q.BM = 256; q.KS = 3; q.SWZ = 2;
  q.halo_bytes = (int)hbs; q.Wp = Wp; q.wg_per_cu = 2;
  q.ntiles = L.Cout / 64;
  q.nblocks = (int)(((long long)L.B * Ho * Wo + 255) / 256) * q.ntiles;
  return finish(q, fast ? "conv3x3s2_fast_kernel<%s>" : "conv3x3s2_split_kernel<%s>");
}

// conv1x1_kernel: stages of CKS 32-channel chunks (wide stages pay once there are several of them); K slices are counted in stages
ConvPlan plan_1x1(const ConvLayer& L, int ksplit) {
  ConvPlan q{};
  const int c32 = L.Cin / 32;
  q.kernel = CK_1X1; q.BM = 256; q.KS = 1; q.SWZ = 1;
  q.CKS = c32 % 4 == 0 ? 4 : (c32 % 2 == 0 ? 2 : 1);
  q.ksplit = ksplit > c32 / q.CKS ? c32 / q.CKS : ksplit;
  q.halo_bytes = 256 * 64; q.Wp = L.Wi;
  q.ntiles = L.Cout / 64;
  q.nblocks = (int)(((long long)L.B * L.Ho() * L.Wo() + 255) / 256) * q.ntiles * q.ksplit;
  return finish(q, "conv1x1_kernel<%s>");
}

// conv_igemm_kernel: 1x1 as a 256-pixel tile; 3x3 with the pixel tile picked so the halo fits, 256 pixels preferred; pooled
// with 256 pixels only where that leaves two workgroups per CU
ConvPlan plan_generic(const ConvLayer& L) {
  ConvPlan q{};
  const bool pool = L.fuse == FUSE_POOL2;
  const int Ho = L.Ho(), Wo = L.Wo(), Hp = L.Hi + 2 * L.pad, Wp = L.Wi + 2 * L.pad, wbytes = L.K * L.K * 4096;
  q.KS = L.K; q.SWZ = L.K == 1 ? 1 : L.stride; q.POOL = pool; q.Wp = Wp; q.BM = 256;
  q.ntiles = L.Cout / 64;
  long long hb = 256 * 64;
  if (L.K == 3) {
    auto bytes = [&](int BM) { return (long long)(pool ? pool_rows_bound(BM, Ho, Wo) : halo_rows_bound(BM, Ho, Wo, Hp, L.stride, 3)) * Wp * 64; };
    hb = bytes(256);
    if (hb + wbytes > (pool ? LDS_HALF : LDS_MAX)) { q.BM = 128; hb = bytes(128); }
    if (pool && (hb + wbytes > LDS_MAX || hb / 64 >= 65536)) return q;
    hb = round1k(hb);
    if (hb + wbytes > LDS_MAX) { snprintf(q.error, sizeof(q.error), "conv_igemm: input rows too wide for LDS (W=%d)", L.Wi); return q; }
    if (hb / 64 >= 65536) { snprintf(q.error, sizeof(q.error), "conv_igemm: halo too large"); return q; }
  }
  q.kernel = CK_IGEMM;
  q.halo_bytes = (int)hb;
  q.nblocks = (int)(((long long)L.B * Ho * Wo + q.BM - 1) / q.BM) * q.ntiles;
  q.layout = pool ? 1 : 0;
  return finish(q, pool ? "conv_igemm_kernel<%s, POOL>" : "conv_igemm_kernel<%s>");
}

// ------------------------------------------------------------------------------------------------
// the cascade (the table in conv_plan.h)
// ------------------------------------------------------------------------------------------------
static ConvPlan plan_pool2(const ConvLayer& L, const ConvTuning& t, int cus, bool inv) {
  ConvPlan q{};
  if (L.B <= 0 || L.Hi <= 0 || L.Wi <= 0 || L.Hi % 2 || L.Wi % 2 || L.Cin <= 0 || L.Cin % 32 || L.Cout <= 0 || L.Cout % 64) return q;
  if ((long long)L.B * L.Hi * L.Wi >= (1ll << 31) || L.Wi + 2 >= 32768 || L.Hi + 2 >= 32768) return q;
  if (L.Cin >= t.pool_min_cin) {
    q = plan_pp_pool(L, t, inv);
    if (q.taken()) return q;
  }
  q = plan_wave(L, t, cus);
  return q.taken() ? q : plan_generic(L);
}

static ConvPlan conv_cascade(const ConvLayer& L, const ConvTuning& t, int cus, bool inv);

// threads of a plan's workgroup (the launchers' block sizes)
static int plan_threads(const ConvPlan& q) { return q.kernel == CK_WAVE || q.kernel >= CK_PP ? 512 : 256; }

ConvPlan conv_plan(const ConvLayer& L, const ConvTuning& t, int cus, bool inv) {
  ConvPlan q{};
  // every kernel numbers output pixels in an int.  The launchers refuse such a layer before they plan; the public queries plan
  // without a launcher in front of them, and the grid arithmetic below is 32-bit
  if ((long long)L.B * L.Ho() * L.Wo() >= (1ll << 31)) {
    snprintf(q.error, sizeof(q.error), "conv_igemm: too many output pixels");
    return q;
  }
  q = conv_cascade(L, t, cus, inv);
  // a grid holds fewer than 2^32 threads (FRMAP_GRID_FITS, frmap_common.h): a larger one is cut down without an error
  if (q.taken() && (long long)q.nblocks * plan_threads(q) >= (1ll << 32)) {
    ConvPlan e{};
    snprintf(e.error, sizeof(e.error), "conv_igemm: %d workgroups of %d threads exceed the grid (shard the batch)", q.nblocks, plan_threads(q));
    return e;
  }
  return q;
}

static ConvPlan conv_cascade(const ConvLayer& L, const ConvTuning& t, int cus, bool inv) {
  ConvPlan q{};
  if (L.fuse == FUSE_POOL2) return plan_pool2(L, t, cus, inv);
  const bool live = t.debug == 0;
  if (L.fuse == FUSE_SHORTCUT && !plan_fast(L, t).taken()) {
    snprintf(q.error, sizeof(q.error), "conv_igemm_ds: this shape does not take the fused-shortcut kernel (check frmap_conv_igemm_ds_supported)");
    return q;
  }
  if (L.K == 1) {
    if (!(live && L.Cin >= 128)) return plan_generic(L);
    q = plan_pp_1x1(L, t, cus, inv);
    return q.taken() ? q : plan_1x1(L, 1);
  }
  if (L.stride == 2 && live) {
    q = plan_pp_s2(L, t, inv);
    if (!q.taken()) q = plan_s2(L, t);
    if (q.taken()) return q;
  }
  if (L.stride == 1 && live) {
    q = plan_pp_3x3(L, t, inv);
    if (q.taken()) return q;
  }
  const ConvPlan g = plan_generic(L);
  if (!g.taken()) return g;
  q = plan_wave(L, t, cus);
  if (!q.taken()) q = plan_fast(L, t);
  return q.taken() ? q : g;
}

// ------------------------------------------------------------------------------------------------
// the fill step (conv_plan.h): after the cascade has decided, on the image-aligned tiles, what runs and in which layout
// ------------------------------------------------------------------------------------------------
ConvPlan conv_fill(const ConvLayer& L, const ConvPlan& q0, const ConvTuning& t, bool inv) {
  if (!t.fill || (q0.kernel != CK_PP && q0.kernel != CK_PP_S2) || q0.PL) return q0;   // switched off; (pooled slices are whole row pairs)
  const bool s2 = q0.kernel == CK_PP_S2;
  const int Ho = s2 ? L.Hi / 2 : L.Hi, Wo = s2 ? L.Wi / 2 : L.Wi, Hp = s2 ? Ho + 1 : Ho + 2;
  const int bn = q0.KS == 2 || q0.WM == 4 ? 128 : 256;
  if (bn == 256) return q0;   // 224 x 256 layouts (>= 200 tiles: 256 faces a stream): measured no faster filled (stride 1 +1.3 %, shortcut -0.4 %, stride 2 +0.7 %)
  // (A/B: FRMAP_PP_FILL >= 2 is a mask of the forms to fill: 2 = 448 x 128 plain / residual, 4 = with the shortcut, 8 = split-K, 16 = stride 2)
  if (t.fill >= 2 && !(t.fill & (s2 ? 16 : (q0.DS ? 4 : (q0.KS == 2 ? 8 : 2))))) return q0;
  const int cap = (q0.KS == 2 || q0.WM == 2 ? 2 : 4) * q0.MI * 16;
  // a forced tile stays, where pp_tile_px applied the value: the hook's everywhere, FRMAP_PP_TILE_PX at stride 1, neither above the capacity
  if ((t.h_px > 0 && t.h_px <= cap) || (!s2 && t.tile_px > 0 && t.tile_px <= cap)) return q0;
  const long long M = (long long)L.B * Ho * Wo;
  // Stride 1 tries the full capacity only: a smaller fill keeps padding MFMAs and still pays the straddle's extra halo pieces
  // (7x7 split-K tiles: 224 pixels would take a seventh piece, 210 fit the six they have and stay out).  Stride 2 has no
  // instantiation for the halo of a full tile (five 8 KB pieces at 28x28): the largest size that fits.
  for (int rows = cap / Wo; rows * Wo > q0.tile_px && (s2 || rows == cap / Wo); --rows) {
    ConvPlan q = q0;
    q.tile_px = rows * Wo;
    q.mtiles = (int)((M + q.tile_px - 1) / q.tile_px);
    const long long hbytes = (long long)pp_max_rows(M, q.tile_px, Ho * Wo, Wo, Hp, s2 ? 2 : 3, inv) * q.Wp * 64;
    if (hbytes / 64 >= 65536) continue;
    q.halo_bytes = (int)hbytes;
    if (s2) {
      q.NHP = pp_s2_nhp_class(hbytes, bn);
      if (!q.NHP) continue;
    } else {
      const int nhp = pp_halo_pieces(hbytes, q.KS);
      if (!nhp || (q.RI && q.KS == 2 && nhp > 4)) continue;                           // (no RI form with 6 halo pieces: keep the form)
      q.NHP = pp_nhp_class(nhp, q.KS, bn, q.DS);
    }
    q = finish(q, q0.label);
    if (q.lds_bytes > LDS_MAX) continue;
    return q;
  }
  return q0;
}

// ------------------------------------------------------------------------------------------------
// the key (conv_plan.h): one name per instantiation, beside the plan fields that select it
// ------------------------------------------------------------------------------------------------
namespace {
enum KeyFlag { F_NONE = 0, F_DS, F_IM, F_PL, F_RI, F_POOL, F_EARLY, F_POOL_EARLY };
struct KeyRow {
  const char* key;
  int kernel, a, b, c, d;   // template arguments in the kernel's order (below); unused ones 0
  int flag;                 // KeyFlag
};
// CK_IGEMM: BM, KS, SWZ | CK_1X1: CKS | CK_WAVE: NCH | CK_PP: MI, WM, NHP, KS | CK_PP_S2: MI, WM, NHP | CK_PP_1X1: MI, WM, KS
const KeyRow KEY_ROWS[] = {
    {"conv_igemm_kernel<256,1,1>", CK_IGEMM, 256, 1, 1, 0, F_NONE},
    {"conv_igemm_kernel<256,3,1>", CK_IGEMM, 256, 3, 1, 0, F_NONE},
    {"conv_igemm_kernel<256,3,2>", CK_IGEMM, 256, 3, 2, 0, F_NONE},
    {"conv_igemm_kernel<128,3,1>", CK_IGEMM, 128, 3, 1, 0, F_NONE},
    {"conv_igemm_kernel<128,3,2>", CK_IGEMM, 128, 3, 2, 0, F_NONE},
    {"conv_igemm_kernel<256,3,1,POOL>", CK_IGEMM, 256, 3, 1, 0, F_POOL},
    {"conv_igemm_kernel<128,3,1,POOL>", CK_IGEMM, 128, 3, 1, 0, F_POOL},
    {"conv1x1_kernel<1>", CK_1X1, 1, 0, 0, 0, F_NONE},
    {"conv1x1_kernel<2>", CK_1X1, 2, 0, 0, 0, F_NONE},
    {"conv1x1_kernel<4>", CK_1X1, 4, 0, 0, 0, F_NONE},
    {"conv3x3_c64_wave_kernel<2>", CK_WAVE, 2, 0, 0, 0, F_NONE},
    {"conv3x3_c64_wave_kernel<2,EARLY>", CK_WAVE, 2, 0, 0, 0, F_EARLY},
    {"conv3x3_c64_wave_kernel<2,POOL>", CK_WAVE, 2, 0, 0, 0, F_POOL},
    {"conv3x3_c64_wave_kernel<2,POOL,EARLY>", CK_WAVE, 2, 0, 0, 0, F_POOL_EARLY},
    {"conv3x3_c64_wave_kernel<1,POOL>", CK_WAVE, 1, 0, 0, 0, F_POOL},
    {"conv3x3_c64_wave_kernel<1,POOL,EARLY>", CK_WAVE, 1, 0, 0, 0, F_POOL_EARLY},
    {"conv3x3_fast_kernel<>", CK_FAST, 0, 0, 0, 0, F_NONE},
    {"conv3x3_fast_kernel<DS>", CK_FAST, 0, 0, 0, 0, F_DS},
    {"conv3x3s2_split_kernel<>", CK_S2_SPLIT, 0, 0, 0, 0, F_NONE},
    {"conv3x3s2_fast_kernel<>", CK_S2_FAST, 0, 0, 0, 0, F_NONE},
    // 224 px x 256 ch
    {"conv3x3_pp_kernel<7,2,3,1>", CK_PP, 7, 2, 3, 1, F_NONE},
    {"conv3x3_pp_kernel<7,2,3,1,DS>", CK_PP, 7, 2, 3, 1, F_DS},
    {"conv3x3_pp_kernel<7,2,3,1,IM>", CK_PP, 7, 2, 3, 1, F_IM},
    {"conv3x3_pp_kernel<7,2,3,1,PL>", CK_PP, 7, 2, 3, 1, F_PL},
    {"conv3x3_pp_kernel<7,2,3,1,RI>", CK_PP, 7, 2, 3, 1, F_RI},
    {"conv3x3_pp_kernel<7,2,5,1>", CK_PP, 7, 2, 5, 1, F_NONE},
    {"conv3x3_pp_kernel<7,2,5,1,DS>", CK_PP, 7, 2, 5, 1, F_DS},
    {"conv3x3_pp_kernel<7,2,5,1,IM>", CK_PP, 7, 2, 5, 1, F_IM},
    {"conv3x3_pp_kernel<7,2,5,1,PL>", CK_PP, 7, 2, 5, 1, F_PL},
    {"conv3x3_pp_kernel<7,2,5,1,RI>", CK_PP, 7, 2, 5, 1, F_RI},
    // 448 px x 128 ch (the shortcut form needs the buffers of NHP = 5: pp_nhp_class)
    {"conv3x3_pp_kernel<7,4,3,1>", CK_PP, 7, 4, 3, 1, F_NONE},
    {"conv3x3_pp_kernel<7,4,3,1,IM>", CK_PP, 7, 4, 3, 1, F_IM},
    {"conv3x3_pp_kernel<7,4,3,1,PL>", CK_PP, 7, 4, 3, 1, F_PL},
    {"conv3x3_pp_kernel<7,4,3,1,RI>", CK_PP, 7, 4, 3, 1, F_RI},
    {"conv3x3_pp_kernel<7,4,5,1>", CK_PP, 7, 4, 5, 1, F_NONE},
    {"conv3x3_pp_kernel<7,4,5,1,DS>", CK_PP, 7, 4, 5, 1, F_DS},
    {"conv3x3_pp_kernel<7,4,5,1,IM>", CK_PP, 7, 4, 5, 1, F_IM},
    {"conv3x3_pp_kernel<7,4,5,1,PL>", CK_PP, 7, 4, 5, 1, F_PL},
    {"conv3x3_pp_kernel<7,4,5,1,RI>", CK_PP, 7, 4, 5, 1, F_RI},
    // split-K 224 px x 128 ch: plain layers only, no RI form with 6 halo pieces (plan_pp_3x3)
    {"conv3x3_pp_kernel<7,2,4,2>", CK_PP, 7, 2, 4, 2, F_NONE},
    {"conv3x3_pp_kernel<7,2,4,2,IM>", CK_PP, 7, 2, 4, 2, F_IM},
    {"conv3x3_pp_kernel<7,2,4,2,RI>", CK_PP, 7, 2, 4, 2, F_RI},
    {"conv3x3_pp_kernel<7,2,6,2>", CK_PP, 7, 2, 6, 2, F_NONE},
    {"conv3x3_pp_kernel<7,2,6,2,IM>", CK_PP, 7, 2, 6, 2, F_IM},
    {"conv3x3s2_pp_kernel<7,2,1>", CK_PP_S2, 7, 2, 1, 0, F_NONE},
    {"conv3x3s2_pp_kernel<7,2,2>", CK_PP_S2, 7, 2, 2, 0, F_NONE},
    {"conv3x3s2_pp_kernel<7,4,1>", CK_PP_S2, 7, 4, 1, 0, F_NONE},
    {"conv3x3s2_pp_kernel<7,4,2>", CK_PP_S2, 7, 4, 2, 0, F_NONE},
    {"conv3x3s2_pp_kernel<7,4,4>", CK_PP_S2, 7, 4, 4, 0, F_NONE},
    {"conv1x1_pp_kernel<7,2,1>", CK_PP_1X1, 7, 2, 1, 0, F_NONE},
    {"conv1x1_pp_kernel<7,4,1>", CK_PP_1X1, 7, 4, 1, 0, F_NONE},
    {"conv1x1_pp_kernel<7,2,2>", CK_PP_1X1, 7, 2, 2, 0, F_NONE},
};
constexpr int N_KEYS = (int)(sizeof(KEY_ROWS) / sizeof(KEY_ROWS[0]));

// a plan in the terms of a row: {kernel, a, b, c, d, flag}; flag -1 = a combination of flags no kernel has
KeyRow row_of(const ConvPlan& q) {
  KeyRow r{"", q.kernel, 0, 0, 0, 0, F_NONE};
  switch (q.kernel) {
    case CK_IGEMM:
      r.a = q.BM; r.b = q.KS; r.c = q.SWZ; r.flag = q.POOL ? F_POOL : F_NONE;
      break;
    case CK_1X1: r.a = q.CKS; break;
    case CK_WAVE:
      r.a = q.NCH; r.flag = q.POOL ? (q.EARLY ? F_POOL_EARLY : F_POOL) : (q.EARLY ? F_EARLY : F_NONE);
      break;
    case CK_FAST: r.flag = q.DS ? F_DS : F_NONE; break;
    case CK_S2_SPLIT: case CK_S2_FAST: break;
    case CK_PP:
      r.a = q.MI; r.b = q.WM; r.c = q.NHP; r.d = q.KS;
      r.flag = (int)q.DS + (int)q.IM + (int)q.PL + (int)q.RI > 1 ? -1 : (q.DS ? F_DS : (q.IM ? F_IM : (q.PL ? F_PL : (q.RI ? F_RI : F_NONE))));
      break;
    case CK_PP_S2: r.a = q.MI; r.b = q.WM; r.c = q.NHP; break;
    case CK_PP_1X1: r.a = q.MI; r.b = q.WM; r.c = q.KS; break;
    default: r.kernel = CK_NONE; break;
  }
  return r;
}
}  // namespace

int conv_plan_key_index(const ConvPlan& q) {
  const KeyRow r = row_of(q);
  if (r.kernel == CK_NONE) return -1;
  for (int i = 0; i < N_KEYS; ++i) {
    const KeyRow& k = KEY_ROWS[i];
    if (k.kernel == r.kernel && k.a == r.a && k.b == r.b && k.c == r.c && k.d == r.d && k.flag == r.flag) return i;
  }
  return -1;
}
const char* conv_plan_key(const ConvPlan& q) {
  const int i = conv_plan_key_index(q);
  return i < 0 ? "" : KEY_ROWS[i].key;
}
int conv_plan_key(const ConvPlan& q, char* buf, int n) {
  const char* key = conv_plan_key(q);
  if (buf && n > 0) snprintf(buf, (size_t)n, "%s", key);
  return (int)strlen(key);
}
const char* const* conv_plan_keys(int* count) {
  static const std::array<const char*, N_KEYS> keys = [] {
    std::array<const char*, N_KEYS> v{};
    for (int i = 0; i < N_KEYS; ++i) v[i] = KEY_ROWS[i].key;
    return v;
  }();
  if (count) *count = N_KEYS;
  return keys.data();
}
bool conv_plan_from_key(const char* key, ConvPlan* q) {
  for (int i = 0; i < N_KEYS; ++i) {
    const KeyRow& k = KEY_ROWS[i];
    if (strcmp(k.key, key)) continue;
    ConvPlan p{};
    p.kernel = k.kernel;
    switch (k.kernel) {
      case CK_IGEMM: p.BM = k.a; p.KS = k.b; p.SWZ = k.c; break;
      case CK_1X1: p.CKS = k.a; break;
      case CK_WAVE: p.NCH = k.a; break;
      case CK_PP: p.MI = k.a; p.WM = k.b; p.NHP = k.c; p.KS = k.d; break;
      case CK_PP_S2: p.MI = k.a; p.WM = k.b; p.NHP = k.c; break;
      case CK_PP_1X1: p.MI = k.a; p.WM = k.b; p.KS = k.c; break;
    }
    p.DS = k.flag == F_DS; p.IM = k.flag == F_IM; p.PL = k.flag == F_PL; p.RI = k.flag == F_RI;
    p.POOL = k.flag == F_POOL || k.flag == F_POOL_EARLY;
    p.EARLY = k.flag == F_EARLY || k.flag == F_POOL_EARLY;
    *q = p;
    return true;
  }
  return false;
}

// FRMAP_DS_UNFUSE_SMALL=1 (A/B switch) answers 0 where the second-generation kernel would take the plain 3x3 layer and the
// maps are small (14x14 / 7x7), so the caller runs the shortcut as its own 1x1 launch and feeds it as the residual.
int conv_ds_supported(const ConvLayer& L, const ConvTuning& t, bool inv) {
  if (!t.dsfuse || L.B <= 0 || L.Hi <= 0 || L.Wi <= 0 || L.Cin <= 0 || L.Cin % 32 || L.Cout <= 0 || L.Cout % 64) return 0;
  if (!plan_fast(L, t).taken()) return 0;
  if (t.ds_unfuse_small && L.Hi * L.Wi <= 256) {
    ConvLayer plain = L;
    plain.fuse = FUSE_NONE;
    if (plan_pp_3x3(plain, t, inv).taken()) return 0;
  }
  return 1;
}

int linear_ksplit(int M, int K, int N, bool inv) {
  const long long tiles = (inv ? 1ll : ((long long)M + 255) / 256) * (N / 64);
  const int nchunks = K / 32;
  int ks = (int)(384 / (tiles > 0 ? tiles : 1));
  if (ks > nchunks / 4) ks = nchunks / 4;
  return ks < 2 ? 1 : ks;
}
