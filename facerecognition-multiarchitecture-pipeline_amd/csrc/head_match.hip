// fp32 heads and gallery matching on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32), gfx950.
//
//   frmap_linear_f32        nn.Linear (+ folded BatchNorm1d) (+ReLU)   face_models.py:32-33,75,467-468,488,678
//   frmap_l2_normalize_f32  F.normalize(p=2, dim=1, eps)               face_models.py:179,525,590
//   frmap_match_top1        compare_faces' arg-min over the gallery    app.py:58-63
//   frmap_match_topk        the k nearest rows / identities, exact      (top-k search)
//   frmap_verify_counts     exact genuine / impostor pair counts per threshold (verification ROC)
//   frmap_match_radius      every pair within a threshold, with its exact distance (watch lists, duplicate enrolments: app.py:428-436)
//   frmap_cosine_logits     class-centre cosine logits + arg-max       hyperparameter_tuning.py:1038-1046
//   frmap_arcmargin_eval    ArcMarginProduct.forward, eval mode        face_models.py:351-429
//
// All four GEMM-shaped ops share one NT kernel  C[b][n] = sum_k A[b][k] * W[n][k]  (both operands
// K-contiguous, like nn.Linear): 256 threads, tile 64 rows x 128 cols, K staged 32 at a time in LDS
// (pitch 33 floats -> conflict-free column reads), wave w owns columns [32w, 32w+32) and both
// 32-row halves.  fp32 in, fp32 accumulate: bitwise an fmaf chain, so arg-min / arg-max decisions
// are taken on true fp32 scores.
//
// The matcher's device code (records, bounds, the exact re-score, the pair feed of the verification counts and the threshold search)
// and its interface to the split-fp16 match GEMM of conv_pp.hip are in match_device.h; the workspace of every match operation is
// laid out by one function here (top1_ws, topk_ws, verify_ws, radius_ws), which its *_workspace_bytes and its entry points share.
#include "match_device.h"
#include "match_scale_rule.h"
#include <type_traits>

enum { MODE_LINEAR = 0, MODE_COS = 1, MODE_ARC = 2, MODE_DIST = 3 };

struct GemmEpi {
  // LINEAR
  const float* scale;
  const float* shift;
  int relu;
  // COS / ARC
  const float* inv_a;  // [B] 1/max(||a||,eps)
  const float* inv_w;  // [N]
  float s;
  float m;
  int easy;
  const int64_t* label;
  unsigned int* minmax_key;  // [2] ordered-uint keys (max, min) or null
  unsigned long long* argkey;  // [B] packed (score, idx) keys or null
  // DIST
  const float* stat_a;  // [B][2] = (sum x^2, sum x)
  const float* stat_w;  // [N][2]
  MatchRec* recs;       // [4 * gridDim.x][B] candidate records, slot = 32 gallery rows (one wave's columns)
  float* out;           // [B][N] or null
};

static inline int waves_blocks(int rows) { return (rows + 3) / 4; }

__device__ __forceinline__ unsigned int f32_ordered(float f) {
  const unsigned int b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ float f32_unordered(unsigned int k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// min (or max) of `v` over the 32 lanes of this lane's half-wave (half_wave_reduce), and the LOWEST lane of the half holding it
// (half_wave_best).  Four DPP steps inside each 16-lane row (quad xor 1, xor 2, half-mirror, mirror), one cross-row exchange,
// then a ballot + find-first: ~10 instructions per reduced row where a 64-bit (value, index) butterfly took ~30.
template <bool MAX>
__device__ __forceinline__ float half_wave_reduce(float v) {
  auto comb = [](float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); };
  auto dpp = [](float x, auto ctrl) {
    const int i = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, decltype(ctrl)::value, 0xF, 0xF, false));
  };
  float m = v;
  m = comb(m, dpp(m, std::integral_constant<int, 0xB1>{}));   // quad_perm [1,0,3,2]
  m = comb(m, dpp(m, std::integral_constant<int, 0x4E>{}));   // quad_perm [2,3,0,1]
  m = comb(m, dpp(m, std::integral_constant<int, 0x141>{}));  // row_half_mirror
  m = comb(m, dpp(m, std::integral_constant<int, 0x140>{}));  // row_mirror
  return comb(m, __shfl_xor(m, 16, 64));
}
template <bool MAX>
__device__ __forceinline__ float half_wave_best(float v, int lk, int& first_li) {
  const float m = half_wave_reduce<MAX>(v);
  const unsigned long long hit = __ballot(v == m);
  const unsigned half = lk ? (unsigned)(hit >> 32) : (unsigned)hit;
  first_li = __ffs(half) - 1;  // >= 0: the lane(s) that contributed m are in the mask
  return m;
}
// plain minimum over the 32 lanes of this lane's half-wave (no index)
__device__ __forceinline__ float half_wave_min(float v) { return half_wave_reduce<false>(v); }

template <int MODE>
__global__ __launch_bounds__(256) void gemm_nt_f32_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                          int B, int N, int K, GemmEpi ep) {
  constexpr int BMr = 64, BNc = 128, KC = 32, PITCH = KC + 1;
  __shared__ float As[BMr * PITCH];
  __shared__ float Ws[BNc * PITCH];
  __shared__ unsigned long long s_key[4 * BMr];  // arg-min / arg-max keys per (wave, row) before the one atomic per row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.y * BMr, n0 = blockIdx.x * BNc;
  const int li = lane & 31, lk = lane >> 5;

  f32x16_t acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }

  const int srow = tid >> 3, skq = (tid & 7) * 4;  // staging: 32 rows x 8 float4 per pass
  for (int k0 = 0; k0 < K; k0 += KC) {
    float4 va[2], vw[4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int row = b0 + srow + r * 32;
      va[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < B && k0 + skq < K) va[r] = *(const float4*)(A + (size_t)row * K + k0 + skq);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = n0 + srow + r * 32;
      vw[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < N && k0 + skq < K) vw[r] = *(const float4*)(W + (size_t)row * K + k0 + skq);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      float* d = As + (srow + r * 32) * PITCH + skq;
      d[0] = va[r].x; d[1] = va[r].y; d[2] = va[r].z; d[3] = va[r].w;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* d = Ws + (srow + r * 32) * PITCH + skq;
      d[0] = vw[r].x; d[1] = vw[r].y; d[2] = vw[r].z; d[3] = vw[r].w;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KC; kk += 2) {
      const float a0 = As[li * PITCH + kk + lk];
      const float a1 = As[(32 + li) * PITCH + kk + lk];
      const float w = Ws[(wave * 32 + li) * PITCH + kk + lk];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w, acc1, 0, 0, 0);
    }
  }

  // epilogue: lane holds column n = n0 + 32*wave + (lane&31), rows (reg&3)+8*(reg>>2)+4*(lane>>5) (+32 for acc1)
  const int n = n0 + wave * 32 + li;
  const bool nvalid = n < N;
  float cmax = -INFINITY, cmin = INFINITY;
  float wscale = 1.f, wshift = 0.f, winv = 0.f, wn2 = 0.f, wsum = 0.f, wband = 0.f;
  if (nvalid) {
    if (MODE == MODE_LINEAR) {
      wscale = ep.scale ? ep.scale[n] : 1.f;
      wshift = ep.shift ? ep.shift[n] : 0.f;
    } else if (MODE == MODE_DIST) {
      wn2 = ep.stat_w[2 * n];
      wsum = ep.stat_w[2 * n + 1];
      wband = match_band(wn2, (float)K);
    } else {
      winv = ep.inv_w[n];
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int b = b0 + h * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
      const float dot = h ? acc1[r] : acc0[r];
      const bool valid = nvalid && b < B;
      if (MODE == MODE_LINEAR) {
        if (valid) {
          float v = dot * wscale + wshift;
          if (ep.relu) v = frmap_relu(v);
          ep.out[(size_t)b * N + n] = v;
        }
      } else if (MODE == MODE_COS) {
        float v = -INFINITY;
        if (valid) {
          v = dot * ep.inv_a[b] * winv * ep.s;
          if (ep.out) ep.out[(size_t)b * N + n] = v;
        }
        if (ep.argkey) {
          // arg-max over n, first index wins ties: maximise (score, ~n); -inf marks columns / rows outside the problem
          int fl;
          const float best = half_wave_best<true>(v, lk, fl);
          if (li == 0) {
            const int nb = n0 + wave * 32 + fl;
            s_key[wave * BMr + h * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk] =
                (b < B && best > -INFINITY) ? (((unsigned long long)f32_ordered(best) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)nb)) : 0ull;
          }
        }
      } else if (MODE == MODE_ARC) {
        if (valid) {
          const float cosr = dot * ep.inv_a[b] * winv;
          cmax = fmaxf(cmax, cosr);
          cmin = fminf(cmin, cosr);
          const float lo = (float)(-1.0 + 1e-7), hi = (float)(1.0 - 1e-7);
          const float c = fminf(fmaxf(cosr, lo), hi);
          float v = c;
          if (ep.label[b] == (int64_t)n) {
            const float theta = acosf(c);
            if (ep.easy) v = c > 0.f ? cosf(theta + ep.m) : c;
            else v = cosf(fminf((float)(3.14159265358979323846 - 1e-4), theta + ep.m));
          }
          v *= ep.s;
          if (isnan(v) || isinf(v)) v = 0.f;
          ep.out[(size_t)b * N + n] = v;
        }
      } else {  // MODE_DIST: ||a - g + eps||^2 = |a|^2 + |g|^2 - 2 a.g + 2 eps (sum a - sum g) + K eps^2, with its error band
        float L = INFINITY, U = INFINITY;  // columns / rows outside the problem never become candidates
        if (valid) {
          const float eps = 1e-6f, kf = (float)K, keps = kf * eps * eps;
          const float sa2 = ep.stat_a[2 * b];
          const float d2 = match_expanded_d2(sa2, ep.stat_a[2 * b + 1], wn2, wsum, dot, keps);
          const float dl = match_kappa(K) * (match_band(sa2, kf) + wband + keps);
          L = d2 - dl; U = d2 + dl;
          match_unbounded(L, U);   // no finite bound (a squared norm past fp32, NaN): in band, the exact re-score decides
        }
        int fl;
        const float l1 = half_wave_best<false>(L, lk, fl);
        const float l2 = half_wave_min(li == fl ? INFINITY : L);
        const float up = half_wave_min(U);
        if (li == 0 && b < B) {
          MatchRec r; r.lo1 = l1; r.idx = l1 < INFINITY ? n0 + wave * 32 + fl : -1; r.lo2 = l2; r.up = up;
          ep.recs[(size_t)(blockIdx.x * 4 + wave) * B + b] = r;
        }
      }
    }
  }
  if (MODE == MODE_COS && ep.argkey) {
    // the four waves' candidates per row meet in LDS: one atomic per row and workgroup instead of one per row and wave
    __syncthreads();
    if (tid < BMr && b0 + tid < B) {
      unsigned long long key = s_key[tid];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const unsigned long long o = s_key[w * BMr + tid];
        key = o > key ? o : key;
      }
      if (key) atomicMax(ep.argkey + b0 + tid, key);
    }
  }
  if (MODE == MODE_ARC && ep.minmax_key) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cmax = fmaxf(cmax, __shfl_xor(cmax, o, 64));
      cmin = fminf(cmin, __shfl_xor(cmin, o, 64));
    }
    if (lane == 0 && cmax >= cmin) {
      atomicMax(ep.minmax_key, f32_ordered(cmax));
      atomicMin(ep.minmax_key + 1, f32_ordered(cmin));
    }
  }
}

template <int MODE>
static int launch_gemm(const float* A, const float* W, int B, int N, int K, const GemmEpi& ep, hipStream_t st) {
  // (rows ride on the grid's y axis: 65535 tiles of 64)
  FRMAP_REQUIRE((B + 63) / 64 <= 65535, "fp32 GEMM: %d rows exceed the grid (at most %d)", B, 65535 * 64);
  dim3 grid((N + 127) / 128, (B + 63) / 64);
  hipLaunchKernelGGL(gemm_nt_f32_kernel<MODE>, grid, dim3(256), 0, st, A, W, B, N, K, ep);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

// ---- row statistics: one wave per row ------------------------------------------------------------
// mode 0: out[r] = 1 / max(||x_r||, eps)      mode 1: out[2r] = sum x^2, out[2r+1] = sum x
__global__ void row_stats_kernel(const float* __restrict__ x, float* __restrict__ out, int R, int D, int mode, float eps) {
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (r >= R) return;
  float s2 = 0.f, s1 = 0.f;
  for (int k = lane; k < D; k += 64) {
    const float v = x[(size_t)r * D + k];
    s2 += v * v;
    s1 += v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s2 += __shfl_xor(s2, o, 64);
    s1 += __shfl_xor(s1, o, 64);
  }
  if (lane == 0) {
    if (mode == 0) out[r] = 1.0f / frmap_max(sqrtf(s2), eps);
    else { out[2 * r] = s2; out[2 * r + 1] = s1; }
  }
}

__global__ void l2_normalize_kernel(const float* __restrict__ x, float* __restrict__ out, int R, int D, float eps) {
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (r >= R) return;
  float s2 = 0.f;
  for (int k = lane; k < D; k += 64) {
    const float v = x[(size_t)r * D + k];
    s2 += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
  const float denom = frmap_max(sqrtf(s2), eps);
  for (int k = lane; k < D; k += 64) out[(size_t)r * D + k] = x[(size_t)r * D + k] / denom;
}

__global__ void fill_u64_kernel(unsigned long long* p, int n, unsigned long long v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// the end of every top-1 match: row `besti` (-1: none) at distance d, the row or -1 under the threshold, and both packed
__device__ __forceinline__ void match_write_top1(int b, int besti, float d, float thresh, int32_t* __restrict__ idx_out,
                                                 float* __restrict__ dist_out, int32_t* __restrict__ id_thr_out,
                                                 int32_t* __restrict__ packed_out) {
  idx_out[b] = besti; dist_out[b] = d;
  const int idt = (besti >= 0 && d <= thresh) ? besti : -1;
  if (id_thr_out) id_thr_out[b] = idt;
  if (packed_out) { packed_out[2 * b] = idt; packed_out[2 * b + 1] = __float_as_int(d); }
}

// One wave per probe.  Reads the probe's candidate records (match_device.h: MatchRec [nslots][B], slot = slot_w consecutive
// gallery rows), takes ug = min over slots of `up`, and re-scores with the exact distance every slot whose lo1 <= ug: the
// slot's single candidate row when its second-best bound lies outside the band, every row of the slot otherwise.  Slots and
// rows are visited in ascending order and only a strictly smaller distance replaces the best one, so the result is the
// FIRST row attaining the minimum of the exact distance: compare_faces' loop (app.py:58-63).
__global__ void match_finalize_rec_kernel(const float* __restrict__ emb, const float* __restrict__ gal,
                                          const MatchRec* __restrict__ recs, int nslots, int slot_w,
                                          int32_t* __restrict__ idx_out, float* __restrict__ dist_out,
                                          int32_t* __restrict__ id_thr_out, int32_t* __restrict__ packed_out, float thresh,
                                          int B, int G, int D) {
  const int b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (b >= B) return;
  const float* a = emb + (size_t)b * D;
  float ug = INFINITY;
  for (int s = lane; s < nslots; s += 64) ug = fminf(ug, recs[(size_t)s * B + b].up);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ug = fminf(ug, __shfl_xor(ug, o, 64));
  double best = INFINITY;
  int besti = -1;
  for (int s0 = 0; s0 < nslots; s0 += 64) {
    MatchRec r; r.lo1 = INFINITY; r.idx = -1; r.lo2 = INFINITY; r.up = INFINITY;
    if (s0 + lane < nslots) r = recs[(size_t)(s0 + lane) * B + b];
    unsigned long long mask = __ballot(r.lo1 <= ug && r.idx >= 0);
    while (mask) {
      const int l = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int ci = __shfl(r.idx, l, 64);
      const float l2 = __shfl(r.lo2, l, 64);
      if (l2 <= ug) {
        const int g0 = (s0 + l) * slot_w, g1 = min(g0 + slot_w, G);
        for (int g = g0; g < g1; ++g) {
          const double d = match_exact_d2(a, gal + (size_t)g * D, D, lane);
          if (d < best) { best = d; besti = g; }
        }
      } else {
        const double d = match_exact_d2(a, gal + (size_t)ci * D, D, lane);
        if (d < best) { best = d; besti = ci; }
      }
    }
  }
  if (lane == 0)
    match_write_top1(b, besti, besti >= 0 ? (float)sqrt(best) : INFINITY, thresh, idx_out, dist_out, id_thr_out, packed_out);
}

// Small galleries (the demo's handful of enrolled faces, the 36-ID benchmark gallery): one workgroup per probe walks the gallery
// directly with the exact distance of every other path (match_exact_d2: fp32 elements, squares summed in float64, so a difference
// whose fp32 square would overflow - rows around 2^64 and beyond - still has its finite distance) - no GEMM expansion, no atomics,
// one launch.
__global__ __launch_bounds__(256) void match_small_kernel(const float* __restrict__ emb, const float* __restrict__ gal,
                                                          int32_t* __restrict__ idx_out, float* __restrict__ dist_out,
                                                          int32_t* __restrict__ id_thr_out, int32_t* __restrict__ packed_out,
                                                          float thresh, int B, int G, int D) {
  // wave w scores gallery rows 8w..8w+7, 8(w+4).. (8 rows per pass so their loads are independent); the four waves'
  // (best, index) pairs meet in LDS, lowest index wins ties
  __shared__ double s_best[4];
  __shared__ int s_idx[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double best = INFINITY;
  int besti = 0x7FFFFFFF;
  for (int g0 = wave * 8; g0 < G; g0 += 32) {
    const float* pa[8];
    const float* pg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { pa[j] = emb + (size_t)b * D; pg[j] = gal + (size_t)min(g0 + j, G - 1) * D; }
    double d2[8];
    match_exact_d2_n<8>(pa, pg, D, lane, d2);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (g0 + j < G && d2[j] < best) { best = d2[j]; besti = g0 + j; }  // strict <: first minimum within this wave's rows
  }
  if (lane == 0) { s_best[wave] = best; s_idx[wave] = besti; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (s_best[w] < best || (s_best[w] == best && s_idx[w] < besti)) { best = s_best[w]; besti = s_idx[w]; }
    const bool any = besti != 0x7FFFFFFF;
    match_write_top1(b, any ? besti : -1, any ? (float)sqrt(best) : INFINITY, thresh, idx_out, dist_out, id_thr_out, packed_out);
  }
}

// The whole tail of the ResNet-18 ('cnn') embed-and-match step for small galleries in one launch, one workgroup
// per face: AdaptiveAvgPool2d(1) of the trunk map (face_models.py:100) -> (optional) F.normalize -> the
// compare_faces scan of match_small_kernel.  Replaces avgpool_global + l2_normalize + match_small (3 launches
// of 5-12 us that are pure latency at 256 faces); the embedding only passes through LDS.
template <typename TT>
__global__ __launch_bounds__(256) void gap_norm_match_kernel(const typename TT::elem* __restrict__ map, const float* __restrict__ gal,
                                                             float* __restrict__ emb_out, int32_t* __restrict__ idx_out,
                                                             float* __restrict__ dist_out, int32_t* __restrict__ id_thr_out,
                                                             int32_t* __restrict__ packed_out, float thresh, int normalize,
                                                             float eps, int HW, int C, int G) {
  extern __shared__ float s_e[];  // [C] embedding, then 4 + 4 reduction slots
  float* s_red = s_e + C;
  int* s_idx = (int*)(s_red + 4);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const typename TT::elem* src = map + (size_t)b * HW * C;
  // pooling: the C/8 8-channel groups x `nparts` interleaved row subsets over the 256 threads, partial sums meet in LDS
  const int C8 = C >> 3, nparts = C8 < 256 ? 256 / C8 : 1;
  float* s_part = s_e + C + 8;  // [nparts][C]
  auto pool_group = [&](int c8, int part) {
    float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int s = part;
    for (; s + 15 * nparts < HW; s += 16 * nparts) {  // sixteen independent 16-byte loads in flight
      u32x4_t r[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) r[q] = *(const u32x4_t*)(src + (size_t)(s + q * nparts) * C + c8 * 8);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float f[8];
        unpack8<TT>(r[q], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += f[j];
      }
    }
    {  // the last (< 16) rows of this subset: loads first (rows past the end re-read the last one and are replaced by zeros:
       // a select, not a weight of 0 - the last row may hold an infinity, and inf * 0 = NaN)
      u32x4_t r[16];
      const int n = s < HW ? (HW - 1 - s) / nparts + 1 : 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) r[q] = *(const u32x4_t*)(src + (size_t)min(s + q * nparts, HW - 1) * C + c8 * 8);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float f[8];
        unpack8<TT>(q < n ? r[q] : (u32x4_t){0u, 0u, 0u, 0u}, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += f[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_part[part * C + c8 * 8 + j] = a[j];
  };
  if (C8 < 256) {
    if (tid < C8 * nparts) pool_group(tid % C8, tid / C8);
  } else {
    for (int c8 = tid; c8 < C8; c8 += 256) pool_group(c8, 0);
  }
  __syncthreads();
  float ss = 0.f;
  {
    const float inv = 1.0f / (float)HW;
    for (int k = tid; k < C; k += 256) {
      float v = 0.f;
      for (int q = 0; q < nparts; ++q) v += s_part[q * C + k];
      v *= inv;
      s_e[k] = v;
      ss += v * v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) s_red[wave] = ss;
  __syncthreads();
  if (normalize) {
    const float denom = frmap_max(sqrtf(s_red[0] + s_red[1] + s_red[2] + s_red[3]), eps);
    for (int k = tid; k < C; k += 256) s_e[k] = s_e[k] / denom;
    __syncthreads();
  }
  if (emb_out)
    for (int k = tid; k < C; k += 256) emb_out[(size_t)b * C + k] = s_e[k];
  // compare_faces scan (as match_small_kernel): wave w scores rows 8w..8w+7, 8(w+4)..; first strict minimum wins
  float best = INFINITY;
  int besti = 0x7FFFFFFF;
  constexpr int RPW = 10;   // gallery rows per wave and pass: 40 rows per pass (the 36-ID gallery in one)
  for (int g0 = 0; g0 < G; g0 += 4 * RPW) {  // this pass: rows g0 + wave, g0 + wave + 4, ...
    // lane l owns dims 8 l .. 8 l + 7 of every 512-dim block: all of a pass's gallery reads (10 rows x 2 x 16 bytes per block)
    // are issued before the first use - one L2 round trip per pass instead of one per 64 dims
    float s2[RPW];
#pragma unroll
    for (int j = 0; j < RPW; ++j) s2[j] = 0.f;
    for (int kk = lane * 8; kk < C; kk += 512) {
      f32x4_t r[RPW][2];
#pragma unroll
      for (int j = 0; j < RPW; ++j) {
        const float* gp = gal + (size_t)min(g0 + 4 * j + wave, G - 1) * C + kk;
        r[j][0] = *(const f32x4_t*)gp;
        r[j][1] = *(const f32x4_t*)(gp + 4);
      }
      const f32x4_t e0 = *(const f32x4_t*)(s_e + kk), e1 = *(const f32x4_t*)(s_e + kk + 4);
#pragma unroll
      for (int j = 0; j < RPW; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float d0 = (e0[c] - r[j][0][c]) + 1e-6f, d1 = (e1[c] - r[j][1][c]) + 1e-6f;
          s2[j] = fmaf(d0, d0, s2[j]);
          s2[j] = fmaf(d1, d1, s2[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < RPW; ++j) {  // ascending row index within the wave: strict < keeps the first minimum
      float v = s2[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      const int gi = g0 + 4 * j + wave;
      if (gi < G && v < best) { best = v; besti = gi; }
    }
  }
  __syncthreads();  // (s_red is reused)
  if (lane == 0) { s_red[wave] = best; s_idx[wave] = besti; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (s_red[w] < best || (s_red[w] == best && s_idx[w] < besti)) { best = s_red[w]; besti = s_idx[w]; }
    const bool any = besti != 0x7FFFFFFF;
    match_write_top1(b, any ? besti : -1, any ? sqrtf(best) : INFINITY, thresh, idx_out, dist_out, id_thr_out, packed_out);
  }
}

extern "C" int frmap_gap_norm_match(const void* map, const float* gallery, float* emb_out, int32_t* idx_out, float* dist_out,
                                    int32_t* id_or_unknown_out, int32_t* packed_out, float thresh, int normalize, float eps,
                                    int B, int HW, int C, int G, int dtype, void* stream) {
  FRMAP_REQUIRE(map && idx_out && dist_out, "gap_norm_match: null pointer");
  FRMAP_REQUIRE(dtype == FRMAP_BF16 || dtype == FRMAP_F16, "gap_norm_match: bad dtype");
  FRMAP_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 8 == 0 && C <= 4096, "gap_norm_match: bad shape B=%d HW=%d C=%d", B, HW, C);
  FRMAP_REQUIRE(B <= FRMAP_GRID_WG256_MAX, "gap_norm_match: %d faces exceed the grid (at most %d)", B, FRMAP_GRID_WG256_MAX);
  FRMAP_REQUIRE(G >= 0 && G <= 64 && (G == 0 || gallery), "gap_norm_match: gallery of 0..64 rows expected (got %d)", G);
  // the map and the gallery rows (C % 8 == 0) are read in 16-byte pieces; every output is written element by element
  FRMAP_REQUIRE_ALIGNED(map, 16, "map");
  FRMAP_REQUIRE_ALIGNED(gallery, 16, "gallery");
  FRMAP_REQUIRE_ALIGNED(emb_out, 4, "emb_out");
  FRMAP_REQUIRE_ALIGNED(idx_out, 4, "idx_out");
  FRMAP_REQUIRE_ALIGNED(dist_out, 4, "dist_out");
  FRMAP_REQUIRE_ALIGNED(id_or_unknown_out, 4, "id_or_unknown_out");
  FRMAP_REQUIRE_ALIGNED(packed_out, 4, "packed_out");
  const int c8 = C / 8, nparts = c8 < 256 ? 256 / c8 : 1;
  const size_t lds = (size_t)(C + 8 + nparts * C) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FRMAP_BF16)
    hipLaunchKernelGGL(gap_norm_match_kernel<BF16>, dim3(B), dim3(256), lds, st, (const __bf16*)map, gallery, emb_out, idx_out,
                       dist_out, id_or_unknown_out, packed_out, thresh, normalize, eps, HW, C, G);
  else
    hipLaunchKernelGGL(gap_norm_match_kernel<F16>, dim3(B), dim3(256), lds, st, (const _Float16*)map, gallery, emb_out, idx_out,
                       dist_out, id_or_unknown_out, packed_out, thresh, normalize, eps, HW, C, G);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// ArcFaceNet head in one launch (face_models.py:573-590: `features(x).view(B,-1)` -> `self.embedding` (Linear, no bias)
// -> `self.bn` (BatchNorm1d, eval) -> F.normalize): global average pool of the NHWC trunk map, y = (x . Wt) * scale +
// shift, e = y / max(||y||, eps).  Replaces avgpool_global + linear_f32 + l2_normalize (three launches, 85 us at 1024
// faces, the pooled features and the un-normalised embedding round-tripping through HBM).
// One workgroup = FB faces: their pooled features sit in LDS as [K][FB] (one broadcast 16-byte read feeds 4 faces), thread t
// owns outputs t, t + 256, ..: the K x N weight matrix is read TRANSPOSED ([K][N], row k = 4 N bytes, coalesced) once
// per workgroup out of L2.
// ------------------------------------------------------------------------------------------------
template <typename TT, int FB, int NPT>
__global__ __launch_bounds__(256) void gap_linear_norm_kernel(const typename TT::elem* __restrict__ map, const float* __restrict__ wt,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              float* __restrict__ pre_out, float* __restrict__ emb_out, float eps,
                                                              int B, int HW, int K, int relu, int stagger) {
  constexpr int N = NPT * 256;
  extern __shared__ float s_all[];
  float* s_x = s_all;                 // [K][FB]
  float* s_red = s_all + K * FB;      // [FB][4] sums of squares
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * FB;
  const int C8 = K >> 3;
  const float inv = 1.0f / (float)HW;
  // pooling: wave w takes faces w and w + 4 side by side (two independent accumulator sets: 16 loads of 16 bytes in flight
  // per lane).  K >= 512: lane l owns the 8-channel groups l, l + 64, .. and walks all HW rows, nothing meets in LDS.
  // K < 512 (BaselineNet: 128 channels x 784 pixels): the 64 lanes are K/8 groups x nsub row subsets, whose partial sums
  // meet in LDS (s_part) in a fixed order.
  static_assert(FB == 8, "two faces per wave, four waves");
  const int nsub = C8 >= 64 ? 1 : 64 / C8;
  float* s_part = s_red + FB * 4;   // [FB][nsub][K] (nsub > 1 only)
  {
    const int fa = wave, fb = wave + 4;
    const typename TT::elem* sa = map + (size_t)min(b0 + fa, B - 1) * HW * K;
    const typename TT::elem* sb = map + (size_t)min(b0 + fb, B - 1) * HW * K;
    const int sub = nsub > 1 ? lane / C8 : 0;
    for (int c8 = nsub > 1 ? lane % C8 : lane; c8 < C8 && sub < nsub; c8 += 64) {
      float a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int s0 = sub; s0 < HW; s0 += 8 * nsub) {
        u32x4_t ra[8], rb[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const size_t o = (size_t)min(s0 + q * nsub, HW - 1) * K + c8 * 8;
          ra[q] = *(const u32x4_t*)(sa + o);
          rb[q] = *(const u32x4_t*)(sb + o);
        }
        if (s0 + 7 * nsub < HW) {   // all 8 rows exist (every trip but a subset's last): plain adds
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            float va[8], vb[8];
            unpack8<TT>(ra[q], va);
            unpack8<TT>(rb[q], vb);
#pragma unroll
            for (int j = 0; j < 8; ++j) { a[j] += va[j]; c[j] += vb[j]; }
          }
        } else {   // rows past the end re-read the last one and are replaced by zeros: a select, not a weight of 0 - the last
                   // row may hold an infinity, and inf * 0 = NaN
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            float va[8], vb[8];
            const bool live = s0 + q * nsub < HW;
            unpack8<TT>(live ? ra[q] : (u32x4_t){0u, 0u, 0u, 0u}, va);
            unpack8<TT>(live ? rb[q] : (u32x4_t){0u, 0u, 0u, 0u}, vb);
#pragma unroll
            for (int j = 0; j < 8; ++j) { a[j] += va[j]; c[j] += vb[j]; }
          }
        }
      }
      if (nsub == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s_x[(c8 * 8 + j) * FB + fa] = a[j] * inv;
          s_x[(c8 * 8 + j) * FB + fb] = c[j] * inv;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s_part[((size_t)fa * nsub + sub) * K + c8 * 8 + j] = a[j];
          s_part[((size_t)fb * nsub + sub) * K + c8 * 8 + j] = c[j];
        }
      }
      if (nsub > 1) break;   // (one group per lane)
    }
  }
  __syncthreads();
  if (nsub > 1) {
    for (int i = tid; i < K * FB; i += 256) {
      const int k = i / FB, f = i - k * FB;
      float v = 0.f;
      for (int q = 0; q < nsub; ++q) v += s_part[((size_t)f * nsub + q) * K + k];
      s_x[i] = v * inv;
    }
    __syncthreads();
  }
  // ---- y[f][n] = sum_k x[f][k] * wt[k][n]
  float acc[NPT][FB];
#pragma unroll
  for (int j = 0; j < NPT; ++j)
#pragma unroll
    for (int f = 0; f < FB; ++f) acc[j][f] = 0.f;
  // every workgroup reads the same K x N matrix: each starts at its own row block so that they do not all pull the same
  // L2 lines at the same time (stagger = 0 under batch-invariant planning: the summation order must not depend on where in
  // the batch a face sits)
  const int kstart = (int)(((long long)blockIdx.x * stagger) % (K / 8)) * 8;
  auto krow = [&](int it) { return it + kstart < K ? it + kstart : it + kstart - K; };
  float wc[8][NPT], wn[8][NPT];
  auto load_w = [&](float (&w)[8][NPT], int k0) {
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < NPT; ++j) w[u][j] = wt[(size_t)(k0 + u) * N + j * 256 + tid];
  };
  load_w(wc, krow(0));
  for (int it = 0; it < K; it += 8) {   // the next 8 rows are requested before this block's FMAs (one L2 round trip per block otherwise)
    const int k0 = krow(it);
    load_w(wn, krow(it + 8 < K ? it + 8 : it));
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float x[FB];
#pragma unroll
      for (int f4 = 0; f4 < FB; f4 += 4) {
        const f32x4_t v = *(const f32x4_t*)(s_x + (k0 + u) * FB + f4);
        x[f4] = v[0]; x[f4 + 1] = v[1]; x[f4 + 2] = v[2]; x[f4 + 3] = v[3];
      }
#pragma unroll
      for (int j = 0; j < NPT; ++j)
#pragma unroll
        for (int f = 0; f < FB; ++f) acc[j][f] = fmaf(x[f], wc[u][j], acc[j][f]);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < NPT; ++j) wc[u][j] = wn[u][j];
  }
  // ---- BatchNorm1d (folded to scale / shift), sum of squares per face, normalise
  float ss[FB];
#pragma unroll
  for (int f = 0; f < FB; ++f) ss[f] = 0.f;
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    const int n = j * 256 + tid;
    const float sc = scale ? scale[n] : 1.f, sh = shift ? shift[n] : 0.f;
#pragma unroll
    for (int f = 0; f < FB; ++f) {
      acc[j][f] = acc[j][f] * sc + sh;
      if (relu) acc[j][f] = frmap_relu(acc[j][f]);
      ss[f] += acc[j][f] * acc[j][f];
    }
  }
#pragma unroll
  for (int f = 0; f < FB; ++f) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss[f] += __shfl_xor(ss[f], o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < FB; ++f) s_red[f * 4 + wave] = ss[f];
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < FB; ++f) {
    if (b0 + f >= B) break;
    const float denom = frmap_max(sqrtf(s_red[f * 4] + s_red[f * 4 + 1] + s_red[f * 4 + 2] + s_red[f * 4 + 3]), eps);
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const size_t o = (size_t)(b0 + f) * N + j * 256 + tid;
      if (pre_out) pre_out[o] = acc[j][f];
      if (emb_out) emb_out[o] = acc[j][f] / denom;
    }
  }
}

// wt: the Linear weight TRANSPOSED, fp32 [K][N] (N in {256, 512}); scale / shift: the folded BatchNorm1d or the Linear bias ([N], may
// be NULL); relu = 1: ReLU before the normalisation (BaselineNet: F.relu(self.fc1(pooled)), face_models.py:43-46);
// pre_out / emb_out: [B][N] fp32 un-normalised / unit-norm embeddings (either may be NULL)
extern "C" int frmap_gap_linear_norm(const void* map, const float* wt, const float* scale, const float* shift, float* pre_out,
                                     float* emb_out, float eps, int B, int HW, int K, int N, int relu, int dtype, void* stream) {
  FRMAP_REQUIRE(map && wt && (pre_out || emb_out), "gap_linear_norm: null pointer");
  FRMAP_REQUIRE(dtype == FRMAP_BF16 || dtype == FRMAP_F16, "gap_linear_norm: bad dtype");
  FRMAP_REQUIRE(B > 0 && HW > 0 && K > 0 && K % 8 == 0 && K <= 2048, "gap_linear_norm: bad shape B=%d HW=%d K=%d", B, HW, K);
  FRMAP_REQUIRE(N == 256 || N == 512, "gap_linear_norm: N=%d not supported (256 or 512)", N);
  FRMAP_REQUIRE_ALIGNED(map, 16, "map");
  FRMAP_REQUIRE_ALIGNED(wt, 4, "wt");
  FRMAP_REQUIRE_ALIGNED(scale, 4, "scale");
  FRMAP_REQUIRE_ALIGNED(shift, 4, "shift");
  FRMAP_REQUIRE_ALIGNED(pre_out, 4, "pre_out");
  FRMAP_REQUIRE_ALIGNED(emb_out, 4, "emb_out");
  constexpr int FB = 8;
  const int c8n = K / 8, nsubh = c8n >= 64 ? 1 : 64 / c8n;
  const size_t lds = (size_t)(K * FB + FB * 4 + (nsubh > 1 ? FB * nsubh * K : 0)) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((B + FB - 1) / FB);
  {
    const void* kerns[4] = {(const void*)gap_linear_norm_kernel<BF16, FB, 2>, (const void*)gap_linear_norm_kernel<BF16, FB, 1>,
                            (const void*)gap_linear_norm_kernel<F16, FB, 2>, (const void*)gap_linear_norm_kernel<F16, FB, 1>};
    if (frmap_big_lds(kerns[(dtype == FRMAP_BF16 ? 0 : 2) + (N == 512 ? 0 : 1)], 160 * 1024)) return -2;
  }
#define GLN_GO(TT, ET, NPT)                                                                                                  \
  hipLaunchKernelGGL((gap_linear_norm_kernel<TT, FB, NPT>), grid, dim3(256), lds, st, (const ET*)map, wt, scale, shift, pre_out, \
                     emb_out, eps, B, HW, K, relu, stagger)
  const int stagger = frmap_batch_invariant() ? 0 : 40;
  if (dtype == FRMAP_BF16) { if (N == 512) GLN_GO(BF16, __bf16, 2); else GLN_GO(BF16, __bf16, 1); }
  else { if (N == 512) GLN_GO(F16, _Float16, 2); else GLN_GO(F16, _Float16, 1); }
#undef GLN_GO
  FRMAP_LAUNCH_CHECK();
  return 0;
}

__global__ void argkey_finalize_kernel(const unsigned long long* __restrict__ keys, int32_t* __restrict__ out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = keys[b] ? (int32_t)(0xFFFFFFFFu - (unsigned)(keys[b] & 0xFFFFFFFFull)) : -1;
}

__global__ void minmax_init_kernel(unsigned int* k) {
  k[0] = 0u;           // running max key
  k[1] = 0xFFFFFFFFu;  // running min key
}
__global__ void minmax_finalize_kernel(const unsigned int* k, float* out) {
  out[0] = f32_unordered(k[0]);
  out[1] = f32_unordered(k[1]);
}

// row softmax + arg-max (first maximum), one wave per row: `probs = F.softmax(outputs, dim=1)`,
// `_, predicted = torch.max(outputs, 1)` of the evaluation loop (src/testing.py:278-279)
__global__ void softmax_argmax_kernel(const float* __restrict__ x, float* __restrict__ probs, int32_t* __restrict__ pred,
                                      int R, int C) {
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (r >= R) return;
  float mx = -INFINITY;
  int mi = 0x7FFFFFFF;
  for (int c = lane; c < C; c += 64) {
    const float v = x[(size_t)r * C + c];
    if (v > mx || (v == mx && c < mi)) { mx = v; mi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
  }
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum += __expf(x[(size_t)r * C + c] - mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (probs)
    for (int c = lane; c < C; c += 64) probs[(size_t)r * C + c] = __expf(x[(size_t)r * C + c] - mx) / sum;
  if (pred && lane == 0) pred[r] = mi;
}

// F.pairwise_distance(a, b) row-wise (eps = 1e-6 on the difference) and the Siamese decision
// `pred = dist < thresh` (src/testing.py:175-177)
__global__ void pairwise_distance_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                         float* __restrict__ dist, int32_t* __restrict__ same, float thresh, int R, int D) {
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (r >= R) return;
  float s2 = 0.f;
  for (int k = lane; k < D; k += 64) {
    const float d = (a[(size_t)r * D + k] - b[(size_t)r * D + k]) + 1e-6f;
    s2 += d * d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
  if (lane == 0) {
    const float d = sqrtf(s2);
    dist[r] = d;
    if (same) same[r] = d < thresh ? 1 : 0;
  }
}

extern "C" size_t frmap_head_workspace_bytes(int B, int C) {
  return (size_t)16 * ((size_t)(B > 0 ? B : 0) + (size_t)(C > 0 ? C : 0)) + 256;
}


extern "C" int frmap_linear_f32(const float* x, const float* w, const float* scale, const float* shift, float* out,
                                int B, int K, int N, int relu, void* stream) {
  FRMAP_REQUIRE(x && w && out, "linear_f32: null pointer");
  FRMAP_REQUIRE(B > 0 && K > 0 && N > 0 && K % 4 == 0, "linear_f32: bad shape B=%d K=%d N=%d (K %% 4 == 0)", B, K, N);
  // (gemm_nt_f32_kernel stages both operands with float4 loads)
  FRMAP_REQUIRE_ALIGNED(x, 16, "x");
  FRMAP_REQUIRE_ALIGNED(w, 16, "w");
  FRMAP_REQUIRE_ALIGNED(scale, 4, "scale");
  FRMAP_REQUIRE_ALIGNED(shift, 4, "shift");
  FRMAP_REQUIRE_ALIGNED(out, 4, "out");
  GemmEpi ep = {};
  ep.scale = scale; ep.shift = shift; ep.relu = relu; ep.out = out;
  return launch_gemm<MODE_LINEAR>(x, w, B, N, K, ep, (hipStream_t)stream);
}

extern "C" int frmap_l2_normalize_f32(const float* x, float* out, int B, int D, float eps, void* stream) {
  FRMAP_REQUIRE(x && out, "l2_normalize: null pointer");
  FRMAP_REQUIRE(B > 0 && D > 0, "l2_normalize: bad shape");
  FRMAP_REQUIRE_ALIGNED(x, 4, "x");
  FRMAP_REQUIRE_ALIGNED(out, 4, "out");
  FRMAP_REQUIRE(B <= FRMAP_GRID_ROWS_MAX, "l2_normalize: %d rows exceed the grid (at most %d)", B, FRMAP_GRID_ROWS_MAX);
  hipLaunchKernelGGL(l2_normalize_kernel, dim3(waves_blocks(B)), dim3(256), 0, (hipStream_t)stream, x, out, B, D, eps);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_softmax_argmax(const float* logits, float* probs_out, int32_t* pred_out, int B, int C, void* stream) {
  FRMAP_REQUIRE(logits && (probs_out || pred_out), "softmax_argmax: null pointer");
  FRMAP_REQUIRE(B > 0 && C > 0, "softmax_argmax: bad shape");
  FRMAP_REQUIRE_ALIGNED(logits, 4, "logits");
  FRMAP_REQUIRE_ALIGNED(probs_out, 4, "probs_out");
  FRMAP_REQUIRE_ALIGNED(pred_out, 4, "pred_out");
  FRMAP_REQUIRE(B <= FRMAP_GRID_ROWS_MAX, "softmax_argmax: %d rows exceed the grid (at most %d)", B, FRMAP_GRID_ROWS_MAX);
  hipLaunchKernelGGL(softmax_argmax_kernel, dim3(waves_blocks(B)), dim3(256), 0, (hipStream_t)stream, logits, probs_out, pred_out, B, C);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_pairwise_distance(const float* a, const float* b, float* dist_out, int32_t* same_out, float thresh,
                                       int B, int D, void* stream) {
  FRMAP_REQUIRE(a && b && dist_out, "pairwise_distance: null pointer");
  FRMAP_REQUIRE(B > 0 && D > 0, "pairwise_distance: bad shape");
  FRMAP_REQUIRE_ALIGNED(a, 4, "a");
  FRMAP_REQUIRE_ALIGNED(b, 4, "b");
  FRMAP_REQUIRE_ALIGNED(dist_out, 4, "dist_out");
  FRMAP_REQUIRE_ALIGNED(same_out, 4, "same_out");
  FRMAP_REQUIRE(B <= FRMAP_GRID_ROWS_MAX, "pairwise_distance: %d rows exceed the grid (at most %d)", B, FRMAP_GRID_ROWS_MAX);
  hipLaunchKernelGGL(pairwise_distance_kernel, dim3(waves_blocks(B)), dim3(256), 0, (hipStream_t)stream, a, b, dist_out, same_out, thresh, B, D);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

static size_t align256_sz(size_t n) { return (n + 255) / 256 * 256; }
static size_t ws_count(int n) { return n > 0 ? (size_t)n : 0; }

// workspace of frmap_match_top1 (the fp32 GEMM: slots of 32 rows, one per wave's columns; statistics [.][2]):
//   records [4 * ceil(G / 128)][B] | probe statistics [B][2] | gallery statistics [G][2]
// and of frmap_match_top1_packed (slots of 64 rows; Gpad = G rounded up to 256: the GEMM's padded rows write never-candidate records):
//   records [Gpad / 64][B] | probe statistics [B][4]
struct Top1Ws {
  MatchRec* recs;
  float* stat_a;
  float* stat_w;   // (unpacked only)
  int nslots, slot_w;
  char* end;
};
static Top1Ws top1_ws(void* ws, int B, int G, bool packed) {
  const size_t b = ws_count(B), g = ws_count(G);
  Top1Ws w;
  w.slot_w = packed ? 64 : 32;
  w.nslots = (int)(packed ? (g + 255) / 256 * 4 : (g + 127) / 128 * 4);
  char* c = (char*)ws;
  w.recs = (MatchRec*)c; c += sizeof(MatchRec) * b * w.nslots;
  w.stat_a = (float*)c; c += (packed ? 16 : 8) * b;
  w.stat_w = (float*)c; c += packed ? 0 : 8 * g;
  w.end = c;
  return w;
}
// one size for both: the unpacked layout never has fewer slots, and 8 B bytes more make room for the packed one's wider statistics
extern "C" size_t frmap_match_workspace_bytes(int B, int G) {
  return (size_t)(top1_ws(nullptr, B, G, false).end - (char*)nullptr) + 8 * ws_count(B) + 256;
}

static int match_finalize_rec(const float* emb, const float* gallery, const Top1Ws& w, int32_t* idx_out, float* dist_out,
                              int32_t* id_or_unknown_out, int32_t* packed_out, float thresh, int B, int G, int D, hipStream_t st) {
  hipLaunchKernelGGL(match_finalize_rec_kernel, dim3(waves_blocks(B)), dim3(256), 0, st, emb, gallery, (const MatchRec*)w.recs, w.nslots,
                     w.slot_w, idx_out, dist_out, id_or_unknown_out, packed_out, thresh, B, G, D);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_match_top1(const float* emb, const float* gallery, int32_t* idx_out, float* dist_out,
                                int32_t* id_or_unknown_out, int32_t* packed_out, float thresh, void* workspace,
                                int B, int G, int D, void* stream) {
  FRMAP_REQUIRE(emb && idx_out && dist_out && workspace, "match_top1: null pointer");
  FRMAP_REQUIRE(B > 0 && D > 0 && D % 4 == 0 && G >= 0, "match_top1: bad shape B=%d G=%d D=%d", B, G, D);
  FRMAP_REQUIRE(G == 0 || gallery, "match_top1: null gallery");
  // the GEMM and the exact re-score read probe and gallery rows as float4 (D % 4 == 0); the workspace starts with 16-byte records
  FRMAP_REQUIRE_ALIGNED(emb, 16, "emb");
  FRMAP_REQUIRE_ALIGNED(gallery, 16, "gallery");
  FRMAP_REQUIRE_ALIGNED(idx_out, 4, "idx_out");
  FRMAP_REQUIRE_ALIGNED(dist_out, 4, "dist_out");
  FRMAP_REQUIRE_ALIGNED(id_or_unknown_out, 4, "id_or_unknown_out");
  FRMAP_REQUIRE_ALIGNED(packed_out, 4, "packed_out");
  FRMAP_REQUIRE_ALIGNED(workspace, 16, "workspace");
  // (G <= 64: one workgroup a probe; else one wave a probe and a gallery row)
  FRMAP_REQUIRE(B <= (G <= 64 ? FRMAP_GRID_WG256_MAX : FRMAP_GRID_ROWS_MAX) && G <= FRMAP_GRID_ROWS_MAX, "match_top1: B=%d or G=%d exceeds the grid", B, G);
  hipStream_t st = (hipStream_t)stream;
  if (G > 0 && G <= 64) {
    hipLaunchKernelGGL(match_small_kernel, dim3(B), dim3(256), 0, st, emb, gallery, idx_out, dist_out,
                       id_or_unknown_out, packed_out, thresh, B, G, D);
    FRMAP_LAUNCH_CHECK();
    return 0;
  }
  const Top1Ws w = top1_ws(G > 0 ? workspace : nullptr, B, G, false);   // (G == 0: no slots, no record is read)
  if (G > 0) {
    hipLaunchKernelGGL(row_stats_kernel, dim3(waves_blocks(B)), dim3(256), 0, st, emb, w.stat_a, B, D, 1, 0.f);
    hipLaunchKernelGGL(row_stats_kernel, dim3(waves_blocks(G)), dim3(256), 0, st, gallery, w.stat_w, G, D, 1, 0.f);
    GemmEpi ep = {};
    ep.stat_a = w.stat_a; ep.stat_w = w.stat_w; ep.recs = w.recs;
    if (int rc = launch_gemm<MODE_DIST>(emb, gallery, B, G, D, ep, st)) return rc;
  }
  return match_finalize_rec(emb, gallery, w, idx_out, dist_out, id_or_unknown_out, packed_out, thresh, B, G, D, st);
}

// ------------------------------------------------------------------------------------------------
// Large galleries on the MFMA pipe.  The fp32 GEMM above runs at ~60 TFLOP/s (fp32 MFMA peaks at 1/16 of the 16-bit
// rate): at 1024 probes x 10 000 identities it is 175 us of a 4 ms step.  Here every fp32 operand x is split into two
// fp16 numbers, hi = fp16(S x), lo = fp16(S x - hi) (S = 256 keeps lo out of the fp16 subnormals for |x| >= 2^-11), and
// a.g ~ (a_hi.g_hi + a_hi.g_lo + a_lo.g_hi) / S^2, accumulated in fp32 by ONE K = 3 D GEMM on the 16x16x32 fp16 MFMA
// (relative error ~2^-22, the size of the fp32 GEMM's own rounding).  The epilogue and the exact finalize step are those
// of the fp32 path, so the result has the same contract: first minimum of the expanded distance, exact
// F.pairwise_distance of the winner.  The gallery is split and laid out in the kernel's weight order ONCE per gallery.
// ------------------------------------------------------------------------------------------------
// Each row gets its own power-of-two scale S (match_scale_rule.h: the largest |x| of a row at or above the cut 2^-113 lands in
// [2^13, 2^14), S and 1 / S are finite, normal powers of two for every row): nothing overflows fp16, lo stays out of the fp16
// subnormals for every element within 2^-11 of the row maximum, and scaling by a power of two is exact;
// statistics record of a row: (sum x^2, sum x, 1 / S, band(x) = the row's share of the expanded distance's error bound, match_device.h).

// one wave per row: statistics + (probes) the split row (a_hi | a_hi | a_lo)
__global__ void match_row_prep_kernel(const float* __restrict__ x, float* __restrict__ stat4, _Float16* __restrict__ split3,
                                      int R, int D) {
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (r >= R) return;
  const float* row = x + (size_t)r * D;
  float s2 = 0.f, s1 = 0.f, amax = 0.f;
  for (int k = lane; k < D; k += 64) {
    const float v = row[k];
    s2 += v * v; s1 += v; amax = fmaxf(amax, fabsf(v));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s2 += __shfl_xor(s2, o, 64); s1 += __shfl_xor(s1, o, 64); amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  }
  const float S = frmap_match_row_scale(amax);
  if (lane == 0) {
    stat4[4 * (size_t)r] = s2; stat4[4 * (size_t)r + 1] = s1; stat4[4 * (size_t)r + 2] = 1.0f / S;
    stat4[4 * (size_t)r + 3] = match_band(s2, (float)D);
  }
  if (split3) {
    _Float16* o = split3 + (size_t)r * 3 * D;
    for (int k = lane; k < D; k += 64) {
      const float v = row[k] * S;
      const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
      o[k] = hi; o[D + k] = hi; o[2 * D + k] = lo;
    }
  }
}

__global__ void match_pack_gallery_kernel(const float* __restrict__ gal, const float* __restrict__ stat4, _Float16* __restrict__ out,
                                          size_t e_lo, size_t e_hi, int G, int D) {
  const int nchunks = 3 * D / 32;
  size_t e = e_lo + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; e < e_hi; e += stride) {   // element order of frmap_pack_conv_weight for a 1x1 layer: [row/64][k/32][row%64][slot][8]
    const int j = (int)(e & 7), slot = (int)((e >> 3) & 3), cl = (int)((e >> 5) & 63);
    const size_t rest = e >> 11;
    const int chunk = (int)(rest % nchunks), ntile = (int)(rest / nchunks);
    const int cg = slot ^ (((cl >> 2) & 1) << 1);
    const int k3 = chunk * 32 + cg * 8 + j, row = ntile * 64 + cl;
    const int part = k3 / D, k = k3 - part * D;        // gallery side: (g_hi | g_lo | g_hi)
    float v = 0.f;
    if (row < G) v = gal[(size_t)row * D + k] * (1.0f / stat4[4 * (size_t)row + 2]);   // (S and 1 / S are normal powers of two: 1 / (1 / S) is S)
    const _Float16 hi = (_Float16)v;
    out[e] = part == 1 ? (_Float16)(v - (float)hi) : hi;
  }
}

extern "C" size_t frmap_match_gallery_pack_bytes(int G, int D) {
  if (G <= 0 || D <= 0) return 0;
  return (size_t)((G + 255) / 256 * 256) * 3 * D * sizeof(_Float16);
}

// (re)pack gallery rows [row_lo, row_hi) of a gallery that now holds G rows: statistics of those rows + every 64-row tile they touch.
static int match_pack_rows(const float* gallery, void* packed_out, float* stat_w_out, int row_lo, int row_hi, int G, int D, hipStream_t st) {
  hipLaunchKernelGGL(match_row_prep_kernel, dim3(waves_blocks(row_hi - row_lo)), dim3(256), 0, st, gallery + (size_t)row_lo * D,
                     stat_w_out + 4 * (size_t)row_lo, (_Float16*)nullptr, row_hi - row_lo, D);
  const size_t per_tile = (size_t)(3 * D / 32) * 2048;
  const size_t e_lo = (size_t)(row_lo / 64) * per_tile;
  // through the end of the last tile's 256-row padding group, so that rows G .. Gpad - 1 are (re)written as zeros
  const size_t t_hi = row_hi >= G ? (size_t)((G + 255) / 256 * 4) : (size_t)((row_hi + 63) / 64);
  const size_t e_hi = t_hi * per_tile;
  const size_t n = e_hi - e_lo;
  const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  hipLaunchKernelGGL(match_pack_gallery_kernel, dim3(blocks), dim3(256), 0, st, gallery, (const float*)stat_w_out,
                     (_Float16*)packed_out, e_lo, e_hi, G, D);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

// one-time preparation of a gallery for frmap_match_top1_packed: packed_out (frmap_match_gallery_pack_bytes), stat_w_out [G][4]
extern "C" int frmap_match_pack_gallery(const float* gallery, void* packed_out, float* stat_w_out, int G, int D, void* stream) {
  FRMAP_REQUIRE(gallery && packed_out && stat_w_out, "match_pack_gallery: null pointer");
  FRMAP_REQUIRE(G > 0 && D > 0 && D % 32 == 0, "match_pack_gallery: bad shape G=%d D=%d (D %% 32 == 0)", G, D);
  FRMAP_REQUIRE_ALIGNED(gallery, 4, "gallery");
  FRMAP_REQUIRE_ALIGNED(packed_out, 2, "packed_out");
  FRMAP_REQUIRE_ALIGNED(stat_w_out, 4, "stat_w_out");
  FRMAP_REQUIRE(G <= FRMAP_GRID_ROWS_MAX, "match_pack_gallery: %d rows exceed the grid (at most %d)", G, FRMAP_GRID_ROWS_MAX);
  return match_pack_rows(gallery, packed_out, stat_w_out, 0, G, G, D, (hipStream_t)stream);
}

// incremental enrolment (app.py:428-436 appends one identity): rows [row_lo, row_hi) of the gallery were
// written (appended: row_hi == G, the new row count; or edited in place); only their statistics and 64-row tiles are re-packed.
// packed_out / stat_w_out must have been sized for at least G rows (frmap_match_gallery_pack_bytes(capacity, D), [capacity][4]).
extern "C" int frmap_match_pack_gallery_rows(const float* gallery, void* packed_out, float* stat_w_out, int row_lo, int row_hi,
                                             int G, int D, void* stream) {
  FRMAP_REQUIRE(gallery && packed_out && stat_w_out, "match_pack_gallery_rows: null pointer");
  FRMAP_REQUIRE(G > 0 && D > 0 && D % 32 == 0 && row_lo >= 0 && row_lo < row_hi && row_hi <= G,
                "match_pack_gallery_rows: bad range [%d, %d) of G=%d D=%d", row_lo, row_hi, G, D);
  FRMAP_REQUIRE_ALIGNED(gallery, 4, "gallery");
  FRMAP_REQUIRE_ALIGNED(packed_out, 2, "packed_out");
  FRMAP_REQUIRE_ALIGNED(stat_w_out, 4, "stat_w_out");
  return match_pack_rows(gallery, packed_out, stat_w_out, row_lo, row_hi, G, D, (hipStream_t)stream);
}

// The packed entry points' first step: whether the split-fp16 GEMM takes the shape and, if so, the probe statistics g.stat_a [P][4]
// and fp16 split g.probes3 [P][3 D] (match_row_prep_kernel).  true: the caller launches its mode's GEMM (frmap_match_gemm_*);
// false: nothing was launched and the entry point answers as its unpacked twin does, from the workspace it was given (same exact
// re-score, same answer).
static bool match_packed_prep(const float* a, const FrmapMatchGemm& g, hipStream_t st, int T = 1) {
  if (!frmap_match_gemm_takes(g.P, g.G, g.D, T)) return false;
  hipLaunchKernelGGL(match_row_prep_kernel, dim3(waves_blocks(g.P)), dim3(256), 0, st, a, (float*)g.stat_a, (_Float16*)g.probes3, g.P, g.D);
  return true;
}

// frmap_match_top1 for a prepared gallery (same outputs, same contract).  workspace: frmap_match_workspace_bytes(B, G)
// bytes; probe_split: B * 3 * D fp16 scratch.
extern "C" int frmap_match_top1_packed(const float* emb, const float* gallery, const void* gallery_packed, const float* stat_w,
                                       int32_t* idx_out, float* dist_out, int32_t* id_or_unknown_out, int32_t* packed_out,
                                       float thresh, void* workspace, void* probe_split, int B, int G, int D, void* stream) {
  FRMAP_REQUIRE(emb && gallery && gallery_packed && stat_w && idx_out && dist_out && workspace && probe_split, "match_top1_packed: null pointer");
  FRMAP_REQUIRE(B > 0 && G > 0 && D > 0 && D % 32 == 0, "match_top1_packed: bad shape B=%d G=%d D=%d", B, G, D);
  FRMAP_REQUIRE_ALIGNED(emb, 16, "emb");
  FRMAP_REQUIRE_ALIGNED(gallery, 16, "gallery");
  FRMAP_REQUIRE_ALIGNED(gallery_packed, 16, "gallery_packed");
  FRMAP_REQUIRE_ALIGNED(stat_w, 16, "stat_w");
  FRMAP_REQUIRE_ALIGNED(idx_out, 4, "idx_out");
  FRMAP_REQUIRE_ALIGNED(dist_out, 4, "dist_out");
  FRMAP_REQUIRE_ALIGNED(id_or_unknown_out, 4, "id_or_unknown_out");
  FRMAP_REQUIRE_ALIGNED(packed_out, 4, "packed_out");
  FRMAP_REQUIRE_ALIGNED(workspace, 16, "workspace");
  FRMAP_REQUIRE_ALIGNED(probe_split, 16, "probe_split");
  FRMAP_REQUIRE(B <= FRMAP_GRID_ROWS_MAX, "match_top1_packed: %d probes exceed the grid (at most %d)", B, FRMAP_GRID_ROWS_MAX);
  hipStream_t st = (hipStream_t)stream;
  const Top1Ws w = top1_ws(workspace, B, G, true);
  const FrmapMatchGemm g = {probe_split, gallery_packed, w.stat_a, stat_w, B, G, D};
  if (!match_packed_prep(emb, g, st))
    return frmap_match_top1(emb, gallery, idx_out, dist_out, id_or_unknown_out, packed_out, thresh, workspace, B, G, D, stream);
  if (int rc = frmap_match_gemm_records(g, w.recs, st)) return rc;
  return match_finalize_rec(emb, gallery, w, idx_out, dist_out, id_or_unknown_out, packed_out, thresh, B, G, D, st);
}

// ------------------------------------------------------------------------------------------------
// Exact top-k search (frmap_match_topk[_packed]): the k gallery rows (entry mode) or identities (identity mode: per label, the
// min over its rows; its representative is the first row attaining it) nearest to each probe under the exact distance of
// match_exact_d2, ordered by (d2, row).  Rows whose distance is NaN or +inf are never listed; missing entries are
// (idx -1, dist +inf, label -1).
//
// One wave per probe keeps a sorted k-list, one entry per lane (k <= 64): lane i < k holds the i-th smallest key (d, row)
// and its label; empty entries are (+inf, INT_MAX, -1).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool topk_less(double d1, int r1, double d2, int r2) { return d1 < d2 || (d1 == d2 && r1 < r2); }

// insert the wave-uniform (d, row, lab).  BY_LABEL: one entry per label, replaced only by a smaller key (a strictly smaller
// d, or an equal d at a lower row); lanes [pos, hi) move down by one, the entry that falls off is lane hi - 1's.
template <bool BY_LABEL>
__device__ __forceinline__ void topk_insert(double& ld, int& lr, int& ll, double d, int row, int lab, int k, int lane) {
  int hi = k;
  if (BY_LABEL) {
    const unsigned long long same = __ballot(lane < k && ll == lab);
    if (same) {
      const int e = __ffsll((long long)same) - 1;
      if (!topk_less(d, row, __shfl(ld, e, 64), __shfl(lr, e, 64))) return;
      hi = e + 1;
    }
  }
  const int pos = __popcll(__ballot(lane < k && topk_less(ld, lr, d, row)));
  if (pos >= hi) return;
  const double ud = __shfl_up(ld, 1, 64);
  const int ur = __shfl_up(lr, 1, 64), ul = __shfl_up(ll, 1, 64);
  if (lane > pos && lane < hi) { ld = ud; lr = ur; ll = ul; }
  if (lane == pos) { ld = d; lr = row; ll = lab; }
}

template <bool BY_LABEL>
__device__ __forceinline__ void topk_write(double ld, int lr, int ll, int b, int k, int lane, int32_t* __restrict__ idx_out,
                                           float* __restrict__ dist_out, int32_t* __restrict__ label_out) {
  if (lane < k) {
    const bool any = lr != 0x7FFFFFFF;
    idx_out[(size_t)b * k + lane] = any ? lr : -1;
    dist_out[(size_t)b * k + lane] = any ? (float)sqrt(ld) : INFINITY;
    if (label_out) label_out[(size_t)b * k + lane] = (BY_LABEL && any) ? ll : -1;
  }
}

// Small or unprepared galleries: one wave per probe scores every row exactly, in row order.
template <bool BY_LABEL>
__global__ void match_topk_scan_kernel(const float* __restrict__ emb, const float* __restrict__ gal, const int32_t* __restrict__ labels,
                                       int32_t* __restrict__ idx_out, float* __restrict__ dist_out, int32_t* __restrict__ label_out,
                                       int B, int G, int D, int k) {
  const int b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (b >= B) return;
  const float* a = emb + (size_t)b * D;
  double ld = INFINITY, kth = INFINITY;
  int lr = 0x7FFFFFFF, ll = -1;
  for (int g = 0; g < G; ++g) {
    const double d = match_exact_d2(a, gal + (size_t)g * D, D, lane);
    if (d < INFINITY && d <= kth) {
      topk_insert<BY_LABEL>(ld, lr, ll, d, g, BY_LABEL ? labels[g] : -1, k, lane);
      kth = __shfl(ld, k - 1, 64);
    }
  }
  topk_write<BY_LABEL>(ld, lr, ll, b, k, lane, idx_out, dist_out, label_out);
}

// Prepared galleries: the records of conv1x1_pp_kernel<..., MATCH_TOPR> (match_device.h: MatchRecK [nslots][B]).
//   tau = the k-th smallest listed U (identity mode: the k-th smallest, over distinct labels, of the per-label min of listed U);
//         +inf when the records name fewer than k rows (labels).
//   re-score with match_exact_d2 every listed row with L <= tau, and every row of a slot whose rest bound is <= tau.
// Why this is exact: the k listed rows (distinct labels) behind tau have exact d2 <= their U <= tau, so the k-th answer has
// d2 <= tau; a row with exact d2 <= tau has L <= d2 <= tau, so it is either listed with L <= tau or unlisted in a slot whose
// rest <= its L <= tau - re-scored either way (in identity mode every row attaining its identity's min is among them, so the
// first one is found).  The running k-th exact key tightens the bound as the list fills: a row with L > the k-th exact d2 can
// change nothing.  Slots are visited in ascending order but the k-list orders by (d2, row) itself, so the visiting order
// does not matter.
template <bool BY_LABEL>
__global__ void match_topk_finalize_kernel(const float* __restrict__ emb, const float* __restrict__ gal, const int32_t* __restrict__ labels,
                                           const MatchRecK* __restrict__ recs, int nslots, int32_t* __restrict__ idx_out,
                                           float* __restrict__ dist_out, int32_t* __restrict__ label_out, int B, int G, int D, int k) {
  const int b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (b >= B) return;
  const float* a = emb + (size_t)b * D;
  MatchRecK none;
#pragma unroll
  for (int j = 0; j < MATCH_R; ++j) { none.lo[j] = INFINITY; none.idx[j] = -1; none.up[j] = INFINITY; }
  none.rest = INFINITY;
  // tau: a k-list of upper bounds
  double ld = INFINITY, kth = INFINITY;
  int lr = 0x7FFFFFFF, ll = -1;
  for (int s0 = 0; s0 < nslots; s0 += 64) {
    const MatchRecK r = s0 + lane < nslots ? recs[(size_t)(s0 + lane) * B + b] : none;
#pragma unroll
    for (int j = 0; j < MATCH_R; ++j) {
      unsigned long long mask = __ballot(r.idx[j] >= 0 && (double)r.up[j] <= kth);
      while (mask) {
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const int row = __shfl(r.idx[j], l, 64);
        const double u = (double)__shfl(r.up[j], l, 64);
        if (u <= kth) {
          topk_insert<BY_LABEL>(ld, lr, ll, u, row, BY_LABEL ? labels[row] : -1, k, lane);
          kth = __shfl(ld, k - 1, 64);
        }
      }
    }
  }
  const double tau = kth;
  // exact re-score into the answer's k-list
  ld = INFINITY; kth = INFINITY; lr = 0x7FFFFFFF; ll = -1;
  auto score = [&](int row) {
    const double d = match_exact_d2(a, gal + (size_t)row * D, D, lane);
    if (d < INFINITY && d <= kth) {
      topk_insert<BY_LABEL>(ld, lr, ll, d, row, BY_LABEL ? labels[row] : -1, k, lane);
      kth = __shfl(ld, k - 1, 64);
    }
  };
  for (int s0 = 0; s0 < nslots; s0 += 64) {
    const MatchRecK r = s0 + lane < nslots ? recs[(size_t)(s0 + lane) * B + b] : none;
    const double bound = fmin(tau, kth);
    const bool full = (double)r.rest <= bound;
    unsigned long long mask = __ballot(full);
    while (mask) {
      const int l = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int g0 = (s0 + l) * 64, g1 = min(g0 + 64, G);
      for (int g = g0; g < g1; ++g) score(g);
    }
#pragma unroll
    for (int j = 0; j < MATCH_R; ++j) {
      mask = __ballot(!full && r.idx[j] >= 0 && (double)r.lo[j] <= fmin(tau, kth));
      while (mask) {
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const double lo = (double)__shfl(r.lo[j], l, 64);
        const int row = __shfl(r.idx[j], l, 64);
        if (lo <= fmin(tau, kth)) score(row);
      }
    }
  }
  topk_write<BY_LABEL>(ld, lr, ll, b, k, lane, idx_out, dist_out, label_out);
}

__global__ void fill_i32_kernel(int32_t* p, int n, int32_t v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// workspace of frmap_match_topk[_packed]: [ top-R records [Gpad / 64][B] | probe statistics [B][4] ] or, for k = 1 in entry mode,
// the top-1 path's own workspace (frmap_match_workspace_bytes) - whichever is larger - then the probes' fp16 split [B][3 D].
struct TopkWs {
  MatchRecK* recs;
  float* stat_a;
  void* split;
  int nslots;
  char* end;
};
static TopkWs topk_ws(void* ws, int B, int G, int D) {
  const size_t b = ws_count(B), g = ws_count(G), d = ws_count(D);
  TopkWs w;
  w.nslots = (int)((g + 255) / 256 * 4);
  char* c = (char*)ws;
  w.recs = (MatchRecK*)c; c += align256_sz(sizeof(MatchRecK) * b * w.nslots);
  w.stat_a = (float*)c; c += align256_sz(16 * b);
  char* top1_end = (char*)ws + align256_sz(frmap_match_workspace_bytes(B, G));
  w.split = c > top1_end ? c : top1_end;
  w.end = (char*)w.split + align256_sz(2 * b * 3 * d);
  return w;
}
extern "C" size_t frmap_match_topk_workspace_bytes(int B, int G, int D, int k) {
  (void)k;
  return (size_t)(topk_ws(nullptr, B, G, D).end - (char*)nullptr) + 256;
}

static int topk_check(const char* what, const float* emb, const float* gallery, int32_t* idx_out, float* dist_out, void* workspace,
                      int B, int G, int D, int k) {
  FRMAP_REQUIRE(emb && idx_out && dist_out && workspace, "%s: null pointer", what);
  FRMAP_REQUIRE(k >= 1 && k <= 64, "%s: k=%d out of range (1 <= k <= 64)", what, k);
  FRMAP_REQUIRE(B > 0 && D > 0 && D % 4 == 0 && G >= 0, "%s: bad shape B=%d G=%d D=%d", what, B, G, D);
  FRMAP_REQUIRE(G == 0 || gallery, "%s: null gallery", what);
  FRMAP_REQUIRE_ALIGNED_AS(what, emb, 16, "emb");
  FRMAP_REQUIRE_ALIGNED_AS(what, gallery, 16, "gallery");
  FRMAP_REQUIRE_ALIGNED_AS(what, idx_out, 4, "idx_out");
  FRMAP_REQUIRE_ALIGNED_AS(what, dist_out, 4, "dist_out");
  FRMAP_REQUIRE_ALIGNED_AS(what, workspace, 256, "workspace");
  FRMAP_REQUIRE(B <= FRMAP_GRID_ROWS_MAX && G <= FRMAP_GRID_ROWS_MAX, "%s: B=%d or G=%d exceeds the grid (at most %d rows)", what, B, G,
                FRMAP_GRID_ROWS_MAX);
  return 0;
}

// k = 1 in entry mode IS the top-1 match (same kernels, so bit-identical outputs); label_out gets -1
int frmap_match_topk_fill_labels(int32_t* label_out, int n, hipStream_t st) {
  if (label_out) hipLaunchKernelGGL(fill_i32_kernel, dim3((n + 255) / 256), dim3(256), 0, st, label_out, n, -1);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_match_topk(const float* emb, const float* gallery, const int32_t* labels, int32_t* idx_out, float* dist_out,
                                int32_t* label_out, void* workspace, int B, int G, int D, int k, void* stream) {
  if (int rc = topk_check("match_topk", emb, gallery, idx_out, dist_out, workspace, B, G, D, k)) return rc;
  FRMAP_REQUIRE_ALIGNED(labels, 4, "labels");
  FRMAP_REQUIRE_ALIGNED(label_out, 4, "label_out");
  hipStream_t st = (hipStream_t)stream;
  if (k == 1 && !labels) {
    const int rc = frmap_match_top1(emb, gallery, idx_out, dist_out, nullptr, nullptr, INFINITY, workspace, B, G, D, stream);
    return rc ? rc : frmap_match_topk_fill_labels(label_out, B, st);
  }
  if (labels)
    hipLaunchKernelGGL(match_topk_scan_kernel<true>, dim3(waves_blocks(B)), dim3(256), 0, st, emb, gallery, labels, idx_out, dist_out,
                       label_out, B, G, D, k);
  else
    hipLaunchKernelGGL(match_topk_scan_kernel<false>, dim3(waves_blocks(B)), dim3(256), 0, st, emb, gallery, labels, idx_out, dist_out,
                       label_out, B, G, D, k);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_match_topk_packed(const float* emb, const float* gallery, const void* gallery_packed, const float* stat_w,
                                       const int32_t* labels, int32_t* idx_out, float* dist_out, int32_t* label_out,
                                       void* workspace, int B, int G, int D, int k, void* stream) {
  if (int rc = topk_check("match_topk_packed", emb, gallery, idx_out, dist_out, workspace, B, G, D, k)) return rc;
  FRMAP_REQUIRE(gallery_packed && stat_w, "match_topk_packed: null pointer");
  FRMAP_REQUIRE_ALIGNED(gallery_packed, 16, "gallery_packed");
  FRMAP_REQUIRE_ALIGNED(stat_w, 16, "stat_w");
  FRMAP_REQUIRE_ALIGNED(labels, 4, "labels");
  FRMAP_REQUIRE_ALIGNED(label_out, 4, "label_out");
  FRMAP_REQUIRE(G > 0 && D % 32 == 0, "match_topk_packed: bad shape B=%d G=%d D=%d (G > 0, D %% 32 == 0)", B, G, D);
  hipStream_t st = (hipStream_t)stream;
  const TopkWs w = topk_ws(workspace, B, G, D);
  if (k == 1 && !labels) {
    const int rc = frmap_match_top1_packed(emb, gallery, gallery_packed, stat_w, idx_out, dist_out, nullptr, nullptr, INFINITY,
                                           workspace, w.split, B, G, D, stream);
    return rc ? rc : frmap_match_topk_fill_labels(label_out, B, st);
  }
  const FrmapMatchGemm g = {w.split, gallery_packed, w.stat_a, stat_w, B, G, D};
  if (!match_packed_prep(emb, g, st))
    return frmap_match_topk(emb, gallery, labels, idx_out, dist_out, label_out, workspace, B, G, D, k, stream);
  if (int rc = frmap_match_gemm_records(g, w.recs, st)) return rc;
  if (labels)
    hipLaunchKernelGGL(match_topk_finalize_kernel<true>, dim3(waves_blocks(B)), dim3(256), 0, st, emb, gallery, labels,
                       (const MatchRecK*)w.recs, w.nslots, idx_out, dist_out, label_out, B, G, D, k);
  else
    hipLaunchKernelGGL(match_topk_finalize_kernel<false>, dim3(waves_blocks(B)), dim3(256), 0, st, emb, gallery, labels,
                       (const MatchRecK*)w.recs, w.nslots, idx_out, dist_out, label_out, B, G, D, k);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Verification counts (frmap_verify_counts[_packed]): for every counted pair (i, j) of A x B (cross mode: all; self mode: A = rows
// [row0, row0 + P) of B, pairs with row0 + i < j) and every threshold t_k, whether (float)sqrt(match_exact_d2) <= t_k, split by
// genuine (label_a[i] == label_b[j]) and impostor.  Pairs are counted per bin (first k with dist <= t_k, T if none) and the
// finalize turns the bins into cumulative counts, so every output is an exact integer independent of path, tiling and launch order.
// workspace: bins u64 [2][T + 1] | rescored u64, bad-threshold flag | table t [T], lo [T], hi [T] | probe statistics [P][4] | probe
// split fp16 [P][3 D].
// ------------------------------------------------------------------------------------------------
struct VerifyWs {
  unsigned long long* hist;
  unsigned long long* misc;   // [0] pairs re-scored, [1] 1 = the thresholds broke the contract
  float* tab;
  float* stat_a;
  void* split;
  char* end;
};
static VerifyWs verify_ws(void* ws, int P, int D, int T) {
  const size_t p = ws_count(P), d = ws_count(D), t = T < 1 ? 1 : T > VERIFY_MAX_T ? VERIFY_MAX_T : (size_t)T;
  VerifyWs w;
  char* c = (char*)ws;
  w.hist = (unsigned long long*)c; c += align256_sz(16 * (t + 1));
  w.misc = (unsigned long long*)c; c += 256;
  w.tab = (float*)c; c += align256_sz(12 * t);
  w.stat_a = (float*)c; c += align256_sz(16 * p);
  w.split = c; c += align256_sz(6 * p * d);
  w.end = c;
  return w;
}
extern "C" size_t frmap_verify_workspace_bytes(int P, int Q, int D, int T) {
  (void)Q;
  return (size_t)(verify_ws(nullptr, P, D, T).end - (char*)nullptr) + 256;
}

// one workgroup: zero the bins, check the thresholds (finite, >= 0, strictly ascending) and bracket each one in d2 space:
//   lo_k = the largest fp32 <= t_k^2:          d2 <= lo_k  =>  sqrt(d2) <= t_k (t_k^2 is exact in float64)  =>  (float)sqrt(d2) <= t_k
//   hi_k = the smallest fp32 >= next_up(t_k)^2: d2 > hi_k   =>  sqrt(d2) >= next_up(t_k)                    =>  (float)sqrt(d2) > t_k
__global__ __launch_bounds__(1024) void verify_prep_kernel(const float* __restrict__ thr, int T, float* __restrict__ tab,
                                                           unsigned long long* __restrict__ hist, unsigned long long* __restrict__ misc) {
  __shared__ int bad;
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  for (int i = tid; i < 2 * (T + 1); i += 1024) hist[i] = 0ull;
  __syncthreads();
  for (int k = tid; k < T; k += 1024) {
    const float t = thr[k];
    const bool ok = __builtin_isfinite(t) && t >= 0.f && (k == 0 || t > thr[k - 1]);
    if (!ok) atomicOr(&bad, 1);
    const float u = nextafterf(t, INFINITY);
    tab[k] = t;
    tab[T + k] = __double2float_rd((double)t * (double)t);
    tab[2 * T + k] = __double2float_ru((double)u * (double)u);
  }
  __syncthreads();
  if (tid == 0) { misc[0] = 0ull; misc[1] = (unsigned long long)bad; }
}

// Exact scan: one workgroup = VS_PB rows of A x VS_QB rows of B; each wave scores PAIR_NB pairs at a time with match_exact_d2's
// arithmetic (pair_scan_block) and bins them in the workgroup's LDS histogram.
__global__ __launch_bounds__(256) void verify_scan_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                          const int32_t* __restrict__ lab_a, const int32_t* __restrict__ lab_b,
                                                          int P, int Q, int D, int row0, const float* __restrict__ tab, int T,
                                                          unsigned long long* __restrict__ hist_g) {
  __shared__ unsigned hist[2 * (VERIFY_MAX_T + 1)];
  __shared__ float tl[VERIFY_MAX_T];
  if (pair_block_below_diagonal(blockIdx.x * VS_PB, blockIdx.y * VS_QB, Q, row0)) return;
  const int tid = threadIdx.x;
  const int nb = 2 * (T + 1);
  for (int i = tid; i < nb; i += 256) hist[i] = 0u;
  for (int i = tid; i < T; i += 256) tl[i] = tab[i];
  __syncthreads();
  VerifySink sink = {lab_a, lab_b, tl, hist, T};
  pair_scan_block(A, B, P, Q, D, row0, sink);
  __syncthreads();
  for (int i = tid; i < nb; i += 256)
    if (hist[i]) atomicAdd(hist_g + i, (unsigned long long)hist[i]);
}

// accepted[c][k] = sum of bins 0 .. k of class c (one workgroup per class, 2 bins per thread, Hillis-Steele over the threads);
// every output all-ones when the thresholds broke the contract
__global__ __launch_bounds__(1024) void verify_finalize_kernel(const unsigned long long* __restrict__ hist,
                                                               const unsigned long long* __restrict__ misc, int T,
                                                               unsigned long long* __restrict__ accepted,
                                                               unsigned long long* __restrict__ rescored_out) {
  __shared__ unsigned long long s[1024];
  const int c = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* h = hist + (size_t)c * (T + 1);
  const int k0 = 2 * tid;
  const unsigned long long v0 = k0 < T ? h[k0] : 0ull, v1 = k0 + 1 < T ? h[k0 + 1] : 0ull;
  s[tid] = v0 + v1;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long add = tid >= o ? s[tid - o] : 0ull;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  const unsigned long long before = tid ? s[tid - 1] : 0ull;
  const bool bad = misc[1] != 0ull;
  if (k0 < T) accepted[(size_t)c * T + k0] = bad ? ~0ull : before + v0;
  if (k0 + 1 < T) accepted[(size_t)c * T + k0 + 1] = bad ? ~0ull : before + v0 + v1;
  if (c == 0 && tid == 0 && rescored_out) *rescored_out = bad ? ~0ull : misc[0];
}

static int verify_check(const char* what, const float* a, const int32_t* label_a, int P, const float* b, const int32_t* label_b, int Q,
                        int D, int a_row0, const float* thresholds, int T, uint64_t* accepted_out, void* workspace) {
  FRMAP_REQUIRE(thresholds && accepted_out && workspace, "%s: null pointer", what);
  FRMAP_REQUIRE(T >= 1 && T <= VERIFY_MAX_T, "%s: T=%d thresholds out of range (1 <= T <= %d)", what, T, VERIFY_MAX_T);
  FRMAP_REQUIRE(P >= 0 && Q >= 0 && D > 0 && D % 4 == 0, "%s: bad shape P=%d Q=%d D=%d (D %% 4 == 0)", what, P, Q, D);
  FRMAP_REQUIRE(P == 0 || (a && label_a), "%s: null A or its labels", what);
  FRMAP_REQUIRE(Q == 0 || (b && label_b), "%s: null B or its labels", what);
  FRMAP_REQUIRE_ALIGNED_AS(what, a, 16, "a");
  FRMAP_REQUIRE_ALIGNED_AS(what, label_a, 4, "label_a");
  FRMAP_REQUIRE_ALIGNED_AS(what, b, 16, "b");
  FRMAP_REQUIRE_ALIGNED_AS(what, label_b, 4, "label_b");
  FRMAP_REQUIRE_ALIGNED_AS(what, thresholds, 4, "thresholds");
  FRMAP_REQUIRE_ALIGNED_AS(what, accepted_out, 8, "accepted_out");
  FRMAP_REQUIRE_ALIGNED_AS(what, workspace, 256, "workspace");
  FRMAP_REQUIRE(a_row0 == -1 || (a_row0 >= 0 && (long long)a_row0 + P <= Q),
                "%s: a_row0=%d with P=%d is not a block of B's %d rows (-1: cross mode)", what, a_row0, P, Q);
  return 0;
}

static int verify_finish(const VerifyWs& w, int T, uint64_t* accepted_out, uint64_t* rescored_out, hipStream_t st) {
  hipLaunchKernelGGL(verify_finalize_kernel, dim3(2), dim3(1024), 0, st, (const unsigned long long*)w.hist,
                     (const unsigned long long*)w.misc, T, (unsigned long long*)accepted_out, (unsigned long long*)rescored_out);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

static int verify_scan(const float* a, const int32_t* label_a, int P, const float* b, const int32_t* label_b, int Q, int D, int a_row0,
                       const VerifyWs& w, int T, hipStream_t st) {
  if (P > 0 && Q > 0)
    hipLaunchKernelGGL(verify_scan_kernel, dim3((P + VS_PB - 1) / VS_PB, (Q + VS_QB - 1) / VS_QB), dim3(256), 0, st, a, b, label_a,
                       label_b, P, Q, D, a_row0, (const float*)w.tab, T, w.hist);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_verify_counts(const float* a, const int32_t* label_a, int P, const float* b, const int32_t* label_b, int Q, int D,
                                   int a_row0, const float* thresholds, int T, uint64_t* accepted_out, uint64_t* rescored_out,
                                   void* workspace, void* stream) {
  if (int rc = verify_check("verify_counts", a, label_a, P, b, label_b, Q, D, a_row0, thresholds, T, accepted_out, workspace)) return rc;
  FRMAP_REQUIRE_ALIGNED(rescored_out, 8, "rescored_out");
  FRMAP_REQUIRE((Q + VS_QB - 1) / VS_QB <= 65535, "verify_counts: Q=%d too large for one call (shard B)", Q);
  hipStream_t st = (hipStream_t)stream;
  const VerifyWs w = verify_ws(workspace, P, D, T);
  hipLaunchKernelGGL(verify_prep_kernel, dim3(1), dim3(1024), 0, st, thresholds, T, w.tab, w.hist, w.misc);
  if (int rc = verify_scan(a, label_a, P, b, label_b, Q, D, a_row0, w, T, st)) return rc;
  return verify_finish(w, T, accepted_out, rescored_out, st);
}

extern "C" int frmap_verify_counts_packed(const float* a, const int32_t* label_a, int P, const float* b, const void* b_packed,
                                          const float* stat_w, const int32_t* label_b, int Q, int D, int a_row0, const float* thresholds,
                                          int T, uint64_t* accepted_out, uint64_t* rescored_out, void* workspace, void* stream) {
  if (int rc = verify_check("verify_counts_packed", a, label_a, P, b, label_b, Q, D, a_row0, thresholds, T, accepted_out, workspace))
    return rc;
  FRMAP_REQUIRE(b_packed && stat_w, "verify_counts_packed: null pointer");
  FRMAP_REQUIRE_ALIGNED(b_packed, 16, "b_packed");
  FRMAP_REQUIRE_ALIGNED(stat_w, 16, "stat_w");
  FRMAP_REQUIRE_ALIGNED(rescored_out, 8, "rescored_out");
  FRMAP_REQUIRE(Q > 0 && D % 32 == 0, "verify_counts_packed: bad shape Q=%d D=%d (Q > 0, D %% 32 == 0)", Q, D);
  FRMAP_REQUIRE((Q + VS_QB - 1) / VS_QB <= 65535, "verify_counts_packed: Q=%d too large for one call (shard B)", Q);
  hipStream_t st = (hipStream_t)stream;
  const VerifyWs w = verify_ws(workspace, P, D, T);
  hipLaunchKernelGGL(verify_prep_kernel, dim3(1), dim3(1024), 0, st, thresholds, T, w.tab, w.hist, w.misc);
  const FrmapMatchGemm g = {w.split, b_packed, w.stat_a, stat_w, P, Q, D};
  if (match_packed_prep(a, g, st, T)) {
    const FrmapVerifyGemm v = {a, b, label_a, label_b, w.tab, w.hist, w.misc, a_row0, T};
    if (int rc = frmap_match_gemm_hist(g, v, st)) return rc;
  } else if (int rc = verify_scan(a, label_a, P, b, label_b, Q, D, a_row0, w, T, st)) {
    return rc;
  }
  return verify_finish(w, T, accepted_out, rescored_out, st);
}

// ------------------------------------------------------------------------------------------------
// Threshold search (frmap_match_radius[_packed]): WHICH pairs the verification counts accept at one threshold.  Every counted pair
// (i, j) of A x B (cross / self mode as above; pair_filter 0 = all, 1 = equal labels, 2 = different labels) with
// (float)sqrt(match_exact_d2) <= thresh is listed once as (i, j, dist), in no particular order; count_out[i] and total_out are exact
// whatever the capacity.  workspace: rescored u64 (when the caller passes no rescored_out) | probe statistics [P][4] | probe split
// fp16 [P][3 D].
// ------------------------------------------------------------------------------------------------
struct RadiusWs {
  unsigned long long* misc;
  float* stat_a;
  void* split;
  char* end;
};
static RadiusWs radius_ws(void* ws, int P, int D) {
  const size_t p = ws_count(P), d = ws_count(D);
  RadiusWs w;
  char* c = (char*)ws;
  w.misc = (unsigned long long*)c; c += 256;
  w.stat_a = (float*)c; c += align256_sz(16 * p);
  w.split = c; c += align256_sz(6 * p * d);
  w.end = c;
  return w;
}
extern "C" size_t frmap_match_radius_workspace_bytes(int P, int Q, int D) {
  (void)Q;
  return (size_t)(radius_ws(nullptr, P, D).end - (char*)nullptr) + 256;
}

__global__ void radius_prep_kernel(int32_t* __restrict__ count, int P, unsigned long long* __restrict__ total,
                                   unsigned long long* __restrict__ rescored) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
  for (int i = i0; i < P; i += gridDim.x * blockDim.x) count[i] = 0;
  if (i0 == 0) { *total = 0ull; *rescored = 0ull; }
}

// Exact scan, the shape of verify_scan_kernel (the same pair_scan_block): the accepted pairs are listed by RadiusSink, the GEMM
// path's own emit step.
__global__ __launch_bounds__(256) void radius_scan_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                          const int32_t* __restrict__ lab_a, const int32_t* __restrict__ lab_b,
                                                          int P, int Q, int D, int row0, int filter, RadiusOut o) {
  if (pair_block_below_diagonal(blockIdx.x * VS_PB, blockIdx.y * VS_QB, Q, row0)) return;
  __shared__ int s_obuf[4][3 * RADIUS_OB];
  RadiusSink sink = {o, s_obuf[threadIdx.x >> 6], lab_a, lab_b, filter, 0};
  pair_scan_block(A, B, P, Q, D, row0, sink);
  sink.flush(threadIdx.x & 63);
}

static int radius_check(const char* what, const float* a, const int32_t* label_a, int P, const float* b, const int32_t* label_b, int Q,
                        int D, int a_row0, float thresh, int pair_filter, int32_t* count_out, uint64_t* total_out, int32_t* pair_out,
                        float* dist_out, long long capacity, void* workspace) {
  FRMAP_REQUIRE(total_out && workspace, "%s: null pointer", what);
  FRMAP_REQUIRE(__builtin_isfinite(thresh) && thresh >= 0.f, "%s: thresh must be finite and >= 0", what);
  FRMAP_REQUIRE(pair_filter >= 0 && pair_filter <= 2, "%s: pair_filter=%d (0 all, 1 equal labels, 2 different labels)", what, pair_filter);
  FRMAP_REQUIRE(P >= 0 && Q >= 0 && D > 0 && D % 4 == 0, "%s: bad shape P=%d Q=%d D=%d (D %% 4 == 0)", what, P, Q, D);
  FRMAP_REQUIRE(P == 0 || (a && count_out && (label_a || !pair_filter)), "%s: null A, its labels or count_out", what);
  FRMAP_REQUIRE(Q == 0 || (b && (label_b || !pair_filter)), "%s: null B or its labels", what);
  FRMAP_REQUIRE(capacity >= 0 && (capacity == 0 || (pair_out && dist_out)), "%s: capacity=%lld needs pair_out and dist_out", what, capacity);
  FRMAP_REQUIRE_ALIGNED_AS(what, a, 16, "a");
  FRMAP_REQUIRE_ALIGNED_AS(what, label_a, 4, "label_a");
  FRMAP_REQUIRE_ALIGNED_AS(what, b, 16, "b");
  FRMAP_REQUIRE_ALIGNED_AS(what, label_b, 4, "label_b");
  FRMAP_REQUIRE_ALIGNED_AS(what, count_out, 4, "count_out");
  FRMAP_REQUIRE_ALIGNED_AS(what, total_out, 8, "total_out");
  FRMAP_REQUIRE_ALIGNED_AS(what, pair_out, 8, "pair_out");
  FRMAP_REQUIRE_ALIGNED_AS(what, dist_out, 4, "dist_out");
  FRMAP_REQUIRE_ALIGNED_AS(what, workspace, 256, "workspace");
  FRMAP_REQUIRE(a_row0 == -1 || (a_row0 >= 0 && (long long)a_row0 + P <= Q),
                "%s: a_row0=%d with P=%d is not a block of B's %d rows (-1: cross mode)", what, a_row0, P, Q);
  FRMAP_REQUIRE((Q + VS_QB - 1) / VS_QB <= 65535, "%s: Q=%d too large for one call (shard B)", what, Q);
  return 0;
}

static int radius_prep(int32_t* count_out, int P, uint64_t* total_out, unsigned long long* resc, hipStream_t st) {
  const int blocks = P > 256 * 1024 ? 1024 : P > 256 ? (P + 255) / 256 : 1;
  hipLaunchKernelGGL(radius_prep_kernel, dim3(blocks), dim3(256), 0, st, count_out, P, (unsigned long long*)total_out, resc);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

static int radius_scan(const float* a, const int32_t* label_a, int P, const float* b, const int32_t* label_b, int Q, int D, int a_row0,
                       int pair_filter, const RadiusOut& o, hipStream_t st) {
  if (P > 0 && Q > 0)
    hipLaunchKernelGGL(radius_scan_kernel, dim3((P + VS_PB - 1) / VS_PB, (Q + VS_QB - 1) / VS_QB), dim3(256), 0, st, a, b, label_a,
                       label_b, P, Q, D, a_row0, pair_filter, o);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_match_radius(const float* a, const int32_t* label_a, int P, const float* b, const int32_t* label_b, int Q, int D,
                                  int a_row0, float thresh, int pair_filter, int32_t* count_out, uint64_t* total_out, int32_t* pair_out,
                                  float* dist_out, long long capacity, uint64_t* rescored_out, void* workspace, void* stream) {
  if (int rc = radius_check("match_radius", a, label_a, P, b, label_b, Q, D, a_row0, thresh, pair_filter, count_out, total_out, pair_out,
                            dist_out, capacity, workspace))
    return rc;
  FRMAP_REQUIRE_ALIGNED(rescored_out, 8, "rescored_out");
  hipStream_t st = (hipStream_t)stream;
  const RadiusWs w = radius_ws(workspace, P, D);
  if (int rc = radius_prep(count_out, P, total_out, rescored_out ? (unsigned long long*)rescored_out : w.misc, st)) return rc;
  const RadiusOut o = {count_out, (unsigned long long*)total_out, pair_out, dist_out, capacity, thresh};
  return radius_scan(a, label_a, P, b, label_b, Q, D, a_row0, pair_filter, o, st);
}

extern "C" int frmap_match_radius_packed(const float* a, const int32_t* label_a, int P, const float* b, const void* b_packed,
                                         const float* stat_w, const int32_t* label_b, int Q, int D, int a_row0, float thresh,
                                         int pair_filter, int32_t* count_out, uint64_t* total_out, int32_t* pair_out, float* dist_out,
                                         long long capacity, uint64_t* rescored_out, void* workspace, void* stream) {
  if (int rc = radius_check("match_radius_packed", a, label_a, P, b, label_b, Q, D, a_row0, thresh, pair_filter, count_out, total_out,
                            pair_out, dist_out, capacity, workspace))
    return rc;
  FRMAP_REQUIRE(b_packed && stat_w, "match_radius_packed: null pointer");
  FRMAP_REQUIRE_ALIGNED(b_packed, 16, "b_packed");
  FRMAP_REQUIRE_ALIGNED(stat_w, 16, "stat_w");
  FRMAP_REQUIRE_ALIGNED(rescored_out, 8, "rescored_out");
  FRMAP_REQUIRE(Q > 0 && D % 32 == 0, "match_radius_packed: bad shape Q=%d D=%d (Q > 0, D %% 32 == 0)", Q, D);
  hipStream_t st = (hipStream_t)stream;
  const RadiusWs w = radius_ws(workspace, P, D);
  unsigned long long* resc = rescored_out ? (unsigned long long*)rescored_out : w.misc;
  if (int rc = radius_prep(count_out, P, total_out, resc, st)) return rc;
  const RadiusOut o = {count_out, (unsigned long long*)total_out, pair_out, dist_out, capacity, thresh};
  // the bracket of verify_prep_kernel, for one threshold known on the host: d2 > hi => sqrt(d2) >= next_up(thresh) => dist > thresh
  const double u = (double)nextafterf(thresh, INFINITY), u2 = u * u;
  float hi = (float)u2;
  if ((double)hi < u2) hi = nextafterf(hi, INFINITY);
  const FrmapMatchGemm g = {w.split, b_packed, w.stat_a, stat_w, P, Q, D};
  if (!match_packed_prep(a, g, st)) return radius_scan(a, label_a, P, b, label_b, Q, D, a_row0, pair_filter, o, st);
  const FrmapRadiusGemm r = {a, b, label_a, label_b, o, resc, hi, a_row0, pair_filter};
  return frmap_match_gemm_join(g, r, st);
}

extern "C" int frmap_cosine_logits(const float* x, const float* w, float* logits_out, int32_t* argmax_out,
                                   void* workspace, int B, int C, int D, float s, void* stream) {
  FRMAP_REQUIRE(x && w && workspace && (logits_out || argmax_out), "cosine_logits: null pointer");
  FRMAP_REQUIRE(B > 0 && C > 0 && D > 0 && D % 4 == 0, "cosine_logits: bad shape");
  FRMAP_REQUIRE_ALIGNED(x, 16, "x");
  FRMAP_REQUIRE_ALIGNED(w, 16, "w");
  FRMAP_REQUIRE_ALIGNED(logits_out, 4, "logits_out");
  FRMAP_REQUIRE_ALIGNED(argmax_out, 4, "argmax_out");
  FRMAP_REQUIRE_ALIGNED(workspace, 16, "workspace");
  FRMAP_REQUIRE(B <= FRMAP_GRID_ROWS_MAX && C <= FRMAP_GRID_ROWS_MAX, "cosine_logits: B=%d or C=%d exceeds the grid (at most %d rows)", B, C, FRMAP_GRID_ROWS_MAX);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  float* inv_a = (float*)(keys + B);
  float* inv_w = inv_a + B;
  hipLaunchKernelGGL(row_stats_kernel, dim3(waves_blocks(B)), dim3(256), 0, st, x, inv_a, B, D, 0, 1e-12f);
  hipLaunchKernelGGL(row_stats_kernel, dim3(waves_blocks(C)), dim3(256), 0, st, w, inv_w, C, D, 0, 1e-12f);
  GemmEpi ep = {};
  ep.inv_a = inv_a; ep.inv_w = inv_w; ep.s = s; ep.out = logits_out;
  if (argmax_out) {
    hipLaunchKernelGGL(fill_u64_kernel, dim3((B + 255) / 256), dim3(256), 0, st, keys, B, 0ull);
    ep.argkey = keys;
  }
  int rc = launch_gemm<MODE_COS>(x, w, B, C, D, ep, st);
  if (rc) return rc;
  if (argmax_out) hipLaunchKernelGGL(argkey_finalize_kernel, dim3((B + 255) / 256), dim3(256), 0, st, keys, argmax_out, B);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_arcmargin_eval(const float* x, const float* w, const int64_t* label, float* logits_out,
                                    float* minmax_out, void* workspace, int B, int C, int D, float s, float m,
                                    int easy_margin, void* stream) {
  FRMAP_REQUIRE(x && w && label && logits_out && workspace, "arcmargin_eval: null pointer");
  FRMAP_REQUIRE(B > 0 && C > 0 && D > 0 && D % 4 == 0, "arcmargin_eval: bad shape");
  FRMAP_REQUIRE_ALIGNED(x, 16, "x");
  FRMAP_REQUIRE_ALIGNED(w, 16, "w");
  FRMAP_REQUIRE_ALIGNED(label, 8, "label");
  FRMAP_REQUIRE_ALIGNED(logits_out, 4, "logits_out");
  FRMAP_REQUIRE_ALIGNED(minmax_out, 4, "minmax_out");
  FRMAP_REQUIRE_ALIGNED(workspace, 16, "workspace");
  FRMAP_REQUIRE(B <= FRMAP_GRID_ROWS_MAX && C <= FRMAP_GRID_ROWS_MAX, "arcmargin_eval: B=%d or C=%d exceeds the grid (at most %d rows)", B, C, FRMAP_GRID_ROWS_MAX);
  hipStream_t st = (hipStream_t)stream;
  unsigned int* mm = (unsigned int*)workspace;
  float* inv_a = (float*)workspace + 4;
  float* inv_w = inv_a + B;
  hipLaunchKernelGGL(row_stats_kernel, dim3(waves_blocks(B)), dim3(256), 0, st, x, inv_a, B, D, 0, 1e-12f);
  hipLaunchKernelGGL(row_stats_kernel, dim3(waves_blocks(C)), dim3(256), 0, st, w, inv_w, C, D, 0, 1e-12f);
  GemmEpi ep = {};
  ep.inv_a = inv_a; ep.inv_w = inv_w; ep.s = s < 24.0f ? s : 24.0f; ep.m = m; ep.easy = easy_margin;
  ep.label = label; ep.out = logits_out;
  if (minmax_out) {
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(1), 0, st, mm);
    ep.minmax_key = mm;
  }
  int rc = launch_gemm<MODE_ARC>(x, w, B, C, D, ep, st);
  if (rc) return rc;
  if (minmax_out) hipLaunchKernelGGL(minmax_finalize_kernel, dim3(1), dim3(1), 0, st, mm, minmax_out);
  FRMAP_LAUNCH_CHECK();
  return 0;
}
