// Shared device/host helpers for the gfx950 kernels.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/frmap_hip.h"
#include "conv_plan.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;

struct BF16 {
  using elem = __bf16;
  using vec8 = bf16x8_t;
  static __device__ __forceinline__ f32x4_t mfma(vec8 a, vec8 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float to_f32(elem v) { return (float)v; }
  static __device__ __forceinline__ elem from_f32(float v) { return (elem)v; }
};
struct F16 {
  using elem = _Float16;
  using vec8 = f16x8_t;
  static __device__ __forceinline__ f32x4_t mfma(vec8 a, vec8 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float to_f32(elem v) { return (float)v; }
  static __device__ __forceinline__ elem from_f32(float v) { return (elem)v; }
};

// pack 4 fp32 -> 4 T (8 bytes)
template <typename TT>
__device__ __forceinline__ u32x2_t pack4(float a, float b, float c, float d) {
  typename TT::elem e[4] = {TT::from_f32(a), TT::from_f32(b), TT::from_f32(c), TT::from_f32(d)};
  u32x2_t r;
  __builtin_memcpy(&r, e, 8);
  return r;
}
template <typename TT>
__device__ __forceinline__ void unpack4(u32x2_t v, float* o) {
  typename TT::elem e[4];
  __builtin_memcpy(e, &v, 8);
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = TT::to_f32(e[i]);
}
template <typename TT>
__device__ __forceinline__ void unpack8(u32x4_t v, float* o) {
  typename TT::elem e[8];
  __builtin_memcpy(e, &v, 16);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = TT::to_f32(e[i]);
}
template <typename TT>
__device__ __forceinline__ u32x4_t pack8(const float* f) {
  typename TT::elem e[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) e[i] = TT::from_f32(f[i]);
  u32x4_t r;
  __builtin_memcpy(&r, e, 16);
  return r;
}

// NaN-propagating maxima (IEEE 754-2019 maximum: NaN if either operand is NaN, maximum(-0, +0) = +0) for every ReLU and
// max-pool between the input and the embedding: `F.relu` and `nn.MaxPool2d` return NaN for a NaN, `fmaxf(NaN, 0)` returns 0
// and the matcher's non-finite guards would never see the value ("Non-finite values").  One v_maximum3_f32 each.
// The matcher's own bound logic keeps fminf / fmaxf: its NaN rules rely on them.
__device__ __forceinline__ float frmap_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float frmap_max3(float a, float b, float c) { return frmap_max(frmap_max(a, b), c); }
__device__ __forceinline__ float frmap_relu(float v) { return frmap_max(v, 0.f); }

// ------------------------------------------------------------------------------------------------
// Top-1 gallery match (compare_faces, /root/reference/src/app.py:58-63) behind a GEMM: candidate records.
//
// The GEMM kernels score a (probe, gallery row) pair by the EXPANDED squared distance
//     d2e = |a|^2 + |g|^2 - 2 a.g + 2 eps (sum a - sum g) + K eps^2        (eps = 1e-6, F.pairwise_distance's)
// whose rounding error is bounded by  delta(a, g) = kappa * (band(a) + band(g) + K eps^2),
//     band(x) = |x|^2 + 2 eps sqrt(K |x|^2)  (>= |x|^2 + 2 eps sum |x_i|),  kappa = (2 T + 64) * 2^-24,
// T = the number of products the dot product accumulates (K for the fp32 GEMM, 3 K for the split-fp16 GEMM whose
// operands carry another 3 * 2^-22 of relative error): a worst-case bound (gamma_T * sum |a_i g_i| <= T u (|a|^2 + |g|^2) / 2
// for the dot product, the same for the two squared norms, a few u for the combination), not a typical-case one.
// So with L = d2e - delta and U = d2e + delta, the row that minimises the EXACT distance has L <= min over all rows of U.
// An epilogue therefore writes, per probe and per SLOT of consecutive gallery rows, one record
//     (lo1, idx) = smallest L of the slot and its row,  lo2 = second smallest L,  up = smallest U
// (no atomics: every record has exactly one writer), and match_finalize_rec_kernel (head_match.hip) re-scores with the exact
// ||(a - g) + eps||_2 every slot whose lo1 <= min up: its single row when lo2 is outside the band, all of its rows otherwise,
// and keeps the first strict minimum - the reference loop's answer, not the expanded form's.
// ------------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) MatchRec {
  float lo1;
  int idx;
  float lo2;
  float up;
};
__device__ __forceinline__ float match_kappa(int terms) { return (float)(2 * terms + 64) * 5.9604644775390625e-8f; }
__device__ __forceinline__ float match_band(float s2, float kf) { return s2 + 2e-6f * sqrtf(kf * s2); }

// Epilogue of the split-fp16 match GEMM (conv1x1_pp_kernel<.., MATCH_TOP1>, frmap_match_gemm): after the K loop lane
// (lr, g) holds, per MFMA tile (mi, ni), the scaled dot products of probe b_base + mi * 16 + lr with gallery rows
// n0 + ni * 16 + 4 g + j.  The wave's 64 gallery rows are one slot (n0 / 64); records are laid out [slot][M].
// Row statistics (match_row_prep_kernel): (sum x^2, sum x, 1 / row scale, band(x)).
template <int MI>
__device__ __forceinline__ void match_epilogue_records(const f32x4_t (&acc)[MI][4], int b_base, int b_end, int n0, int G, int D,
                                                       int M, const float* __restrict__ stat_a,
                                                       const float* __restrict__ stat_w, MatchRec* __restrict__ recs,
                                                       int lane) {
  const int lr = lane & 15, g = lane >> 4;
  const float eps = 1e-6f, kf = (float)D, keps = kf * eps * eps, kap = match_kappa(3 * D);
  // One probe row (mi) at a time; the gallery-row statistics are re-read per (mi, ni) block (L1 hits) instead of being held for
  // the whole epilogue, so the live set stays at acc + ~30 registers: the kernels around this epilogue count their LDS-DMA with
  // s_waitcnt vmcnt(n) and must not spill (csrc/build.sh checks)
  MatchRec* out = recs + (size_t)(n0 >> 6) * M;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int b = b_base + mi * 16 + lr;
    const f32x4_t sa = *(const f32x4_t*)(stat_a + 4 * (size_t)min(b, M - 1));
    const float a2 = sa[0], as = sa[1], ai = sa[2], ab = sa[3] + keps;
    float l1 = INFINITY, l2 = INFINITY, up = INFINITY;
    int i1 = -1;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + ni * 16 + 4 * g + j;
        const f32x4_t sw = *(const f32x4_t*)(stat_w + 4 * (size_t)min(n, G - 1));
        const float d2 = a2 + sw[0] - 2.f * (acc[mi][ni][j] * ai * sw[2]) + 2.f * eps * (as - sw[1]) + keps;
        const float dl = kap * (ab + sw[3]);
        const float L = n < G ? d2 - dl : INFINITY, U = n < G ? d2 + dl : INFINITY;
        if (L < l1) { l2 = l1; l1 = L; i1 = n; }   // rows ascend inside the lane: the first of equal L keeps the index,
        else if (L < l2) l2 = L;                   // the second lands in lo2 (= lo1: the whole slot is re-scored)
        up = fminf(up, U);
      }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float ol1 = __shfl_xor(l1, o, 64), ol2 = __shfl_xor(l2, o, 64), ou = __shfl_xor(up, o, 64);
      const int oi1 = __shfl_xor(i1, o, 64);
      const float nl2 = fminf(fminf(l2, ol2), fmaxf(l1, ol1));
      if (ol1 < l1) { l1 = ol1; i1 = oi1; }
      l2 = nl2; up = fminf(up, ou);
    }
    if (g == 0 && b < b_end) {
      MatchRec r; r.lo1 = l1; r.idx = i1; r.lo2 = l2; r.up = up;
      out[b] = r;
    }
    __builtin_amdgcn_sched_barrier(0);   // one probe row's loads at a time: no hoisting of the next row's statistics loads
  }
}

// ------------------------------------------------------------------------------------------------
// Top-k gallery search behind the same GEMM: per probe and 64-row slot, the R = 4 smallest lower bounds L of the slot (ascending,
// first row first among equal L) with their rows and upper bounds U, and `rest` = the (R+1)-th smallest L, a lower bound on every
// row of the slot that is not listed.  Error bounds as match_epilogue_records.  match_topk_finalize_kernel (head_match.hip) takes
// tau = the k-th smallest listed U (per distinct label in identity mode) and re-scores exactly every listed row with L <= tau and
// every row of a slot whose rest <= tau.  An identity enrolled up to R times in one slot never forces a whole-slot re-score.
// ------------------------------------------------------------------------------------------------
enum MatchMode { MATCH_NONE = 0, MATCH_TOP1 = 1, MATCH_TOPR = 2, MATCH_HIST = 3, MATCH_JOIN = 4 };   // MATCH_HIST: verification counts, MATCH_JOIN: threshold search
constexpr int MATCH_R = 4;
struct __attribute__((aligned(16))) MatchRecK {   // 64 bytes
  float lo[MATCH_R];
  int idx[MATCH_R];   // -1: none
  float up[MATCH_R];
  float rest;
  int pad[3];
};

// insert (L, n, U) into an ascending R-list; what falls off (or L itself) lowers `rest`.  Strict compares: an equal L goes after,
// and a NaN L is never listed nor counted.
__device__ __forceinline__ void match_topr_insert(float (&lo)[MATCH_R], int (&ix)[MATCH_R], float (&up)[MATCH_R], float& rest,
                                                  float L, int n, float U) {
  rest = fminf(rest, L < lo[MATCH_R - 1] ? lo[MATCH_R - 1] : L);
#pragma unroll
  for (int j = MATCH_R - 1; j >= 0; --j) {
    const bool shift = j > 0 && L < lo[j - 1];          // the entry above moves down into slot j
    const bool here = L < lo[j] && !shift;              // L lands in slot j
    if (j > 0 && shift) { lo[j] = lo[j - 1]; ix[j] = ix[j - 1]; up[j] = up[j - 1]; }
    else if (here) { lo[j] = L; ix[j] = n; up[j] = U; }
  }
}

template <int MI>
__device__ __forceinline__ void match_epilogue_topr(const f32x4_t (&acc)[MI][4], int b_base, int b_end, int n0, int G, int D, int M,
                                                    const float* __restrict__ stat_a, const float* __restrict__ stat_w,
                                                    MatchRecK* __restrict__ recs, int lane) {
  const int lr = lane & 15, g = lane >> 4;
  const float eps = 1e-6f, kf = (float)D, keps = kf * eps * eps, kap = match_kappa(3 * D);
  MatchRecK* out = recs + (size_t)(n0 >> 6) * M;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int b = b_base + mi * 16 + lr;
    const f32x4_t sa = *(const f32x4_t*)(stat_a + 4 * (size_t)min(b, M - 1));
    const float a2 = sa[0], as = sa[1], ai = sa[2], ab = sa[3] + keps;
    float lo[MATCH_R], up[MATCH_R], rest = INFINITY;
    int ix[MATCH_R];
#pragma unroll
    for (int j = 0; j < MATCH_R; ++j) { lo[j] = INFINITY; up[j] = INFINITY; ix[j] = -1; }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + ni * 16 + 4 * g + j;
        const f32x4_t sw = *(const f32x4_t*)(stat_w + 4 * (size_t)min(n, G - 1));
        const float d2 = a2 + sw[0] - 2.f * (acc[mi][ni][j] * ai * sw[2]) + 2.f * eps * (as - sw[1]) + keps;
        const float dl = kap * (ab + sw[3]);
        const float L = n < G ? d2 - dl : INFINITY, U = n < G ? d2 + dl : INFINITY;
        match_topr_insert(lo, ix, up, rest, L, n, U);   // rows ascend inside the lane
      }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      float olo[MATCH_R], oup[MATCH_R];
      int oix[MATCH_R];
#pragma unroll
      for (int j = 0; j < MATCH_R; ++j) {
        olo[j] = __shfl_xor(lo[j], o, 64); oup[j] = __shfl_xor(up[j], o, 64); oix[j] = __shfl_xor(ix[j], o, 64);
      }
      rest = fminf(rest, __shfl_xor(rest, o, 64));
#pragma unroll
      for (int j = 0; j < MATCH_R; ++j) match_topr_insert(lo, ix, up, rest, olo[j], oix[j], oup[j]);
    }
    if (g == 0 && b < b_end) {
      MatchRecK r;
#pragma unroll
      for (int j = 0; j < MATCH_R; ++j) { r.lo[j] = lo[j]; r.idx[j] = ix[j]; r.up[j] = up[j]; }
      r.rest = rest; r.pad[0] = r.pad[1] = r.pad[2] = 0;
      out[b] = r;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ||(a - g) + eps||_2^2 the way F.pairwise_distance forms its elements (fp32 subtract, fp32 add of eps), squares summed in
// float64 by the whole wave: the result does not depend on a summation order, identical rows give identical values, and it
// is within 2^-24 of what any fp32 summation of the same 512 squares returns.  Every lane gets the sum.
__device__ __forceinline__ double match_exact_d2(const float* __restrict__ a, const float* __restrict__ g, int D, int lane) {
  double s2 = 0.0;
  for (int k = lane * 4; k < D; k += 256) {
    const f32x4_t av = *(const f32x4_t*)(a + k), gv = *(const f32x4_t*)(g + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = (av[j] - gv[j]) + 1e-6f;
      s2 += (double)d * (double)d;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
  return s2;
}

// NB pairs at once, each summed in exactly match_exact_d2's order (bit-identical results); the NB loads of a k-step are in flight
// together, which is what a wave that re-scores a queue of unrelated pairs (L2 latency, no reuse) needs.
template <int NB>
__device__ __forceinline__ void match_exact_d2_n(const float* const (&a)[NB], const float* const (&g)[NB], int D, int lane,
                                                 double (&out)[NB]) {
#pragma unroll
  for (int q = 0; q < NB; ++q) out[q] = 0.0;
  for (int k = lane * 4; k < D; k += 256) {
    f32x4_t av[NB], gv[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) { av[q] = *(const f32x4_t*)(a[q] + k); gv[q] = *(const f32x4_t*)(g[q] + k); }
#pragma unroll
    for (int q = 0; q < NB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = (av[q][j] - gv[q][j]) + 1e-6f;
        out[q] += (double)d * (double)d;
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int q = 0; q < NB; ++q) out[q] += __shfl_xor(out[q], o, 64);
}

// ------------------------------------------------------------------------------------------------
// Verification counts (frmap_verify_counts[_packed], head_match.hip): every counted pair (i, j) of A x B falls in bin
// k = the first threshold with (float)sqrt(d2) <= t_k (T if none: NaN / inf / beyond the grid), per class (0 = genuine, 1 = impostor).
// Bins are counted per workgroup in LDS (u32 [2][T + 1]) and flushed with one 64-bit atomicAdd per non-zero bin.
// ------------------------------------------------------------------------------------------------
constexpr int VERIFY_MAX_T = 2048;
// LDS layout of the verify workgroups (bytes): histogram u32 [2][T + 1] | t [T] | lo [T] | hi [T] | the GEMM path's per-wave queues
constexpr int VERIFY_LDS_HIST = 0;
constexpr int VERIFY_LDS_T = 16400;                               // >= 8 * (VERIFY_MAX_T + 1), 16-aligned
constexpr int VERIFY_LDS_LO = VERIFY_LDS_T + 4 * VERIFY_MAX_T;
constexpr int VERIFY_LDS_HI = VERIFY_LDS_LO + 4 * VERIFY_MAX_T;
constexpr int VERIFY_LDS_Q = VERIFY_LDS_HI + 4 * VERIFY_MAX_T;
constexpr int VERIFY_QCAP = 7 * 16 * 64;                          // pairs of one match-GEMM wave (MI = 7): the queue never overflows
constexpr int VERIFY_LDS_GEMM = VERIFY_LDS_Q + 8 * VERIFY_QCAP * 2;

// first k in [0, T) with v <= tab[k] (tab ascending), T if none (NaN: T)
__device__ __forceinline__ int verify_bin(const float* tab, int T, float v) {
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v <= tab[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// bin NB pairs whose exact d2 every lane holds: lane q < NB takes pair q (valid[q] false: skipped)
template <int NB>
__device__ __forceinline__ void verify_bin_pairs(const double (&d2)[NB], const bool (&valid)[NB], const bool (&gen)[NB],
                                                 const float* t_lds, unsigned* hist_lds, int T, int lane) {
  double d = 0.0;
  bool v = false, ge = false;
#pragma unroll
  for (int q = 0; q < NB; ++q)
    if (lane == q) { d = d2[q]; v = valid[q]; ge = gen[q]; }
  if (v) {
    const float dist = (float)sqrt(d);
    atomicAdd(hist_lds + (ge ? 0 : T + 1) + verify_bin(t_lds, T, dist), 1u);
  }
}

// Epilogue of conv1x1_pp_kernel<..., MATCH_HIST>: pair (probe b = A row, gallery row n = B row) has L <= d2 <= U (bounds as
// match_epilogue_topr).  With the host's brackets (d2 <= lo_k => dist <= t_k, d2 > hi_k => dist > t_k, both ascending) the pair's
// bin is certain when kU = the first k with U <= lo_k has L > hi_{kU - 1} (or kU = 0), with L and U finite: then d2 <= lo_kU and
// d2 > hi_k for every k < kU.  Certain pairs are binned at once; the others go to this wave's LDS queue (u16 = the pair's place in
// the wave's 112 x 64 block) and are re-scored with match_exact_d2 by verify_drain_queue.  Returns the queue length (wave-uniform).
template <int MI>
__device__ __forceinline__ int match_epilogue_hist(const f32x4_t (&acc)[MI][4], int b_base, int b_end, int n0, int G, int D, int M,
                                                   const float* __restrict__ stat_a, const float* __restrict__ stat_w,
                                                   const int32_t* __restrict__ lab_a, const int32_t* __restrict__ lab_b, int row0,
                                                   const float* lo_lds, const float* hi_lds, unsigned* hist_lds,
                                                   unsigned short* queue, int T, int lane) {
  const int lr = lane & 15, g = lane >> 4;
  const float eps = 1e-6f, kf = (float)D, keps = kf * eps * eps, kap = match_kappa(3 * D);
  int cnt = 0;
  // a lane's certain pairs mostly land in the same bin as the one before (every lane of the wave, often in the same bin): runs
  // are merged in registers and added with one LDS atomic per run instead of one per pair (64-way serialised on a shared bin)
  int rk = 0;
  unsigned rn = 0u;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int b = b_base + mi * 16 + lr;
    const f32x4_t sa = *(const f32x4_t*)(stat_a + 4 * (size_t)min(b, M - 1));
    const float a2 = sa[0], as = sa[1], ai = sa[2], ab = sa[3] + keps;
    const int la = lab_a[min(b, M - 1)];
    const int nmin = row0 >= 0 ? row0 + b + 1 : 0;   // self mode: only rows after the probe's own
    // re-read the gallery rows' statistics and labels per probe row: opaque copies of the pointers keep the compiler from merging
    // the 16 rows' loads of all MI probe rows into one set held across the whole epilogue (~80 registers next to acc)
    const float* sw_p = stat_w;
    const int32_t* lb_p = lab_b;
    asm volatile("" : "+s"(sw_p), "+s"(lb_p));
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + ni * 16 + 4 * g + j;
        const f32x4_t sw = *(const f32x4_t*)(sw_p + 4 * (size_t)min(n, G - 1));
        const float d2 = a2 + sw[0] - 2.f * (acc[mi][ni][j] * ai * sw[2]) + 2.f * eps * (as - sw[1]) + keps;
        const float dl = kap * (ab + sw[3]);
        const float L = d2 - dl, U = d2 + dl;
        const bool valid = n < G && b < b_end && n >= nmin;
        bool sure = false;
        if (valid) {
          const int k = verify_bin(lo_lds, T, U);
          sure = __builtin_isfinite(L) && __builtin_isfinite(U) && (k == 0 || L > hi_lds[k - 1]);
          if (sure) {
            const int key = (la == lb_p[min(n, G - 1)] ? 0 : T + 1) + k;
            if (key != rk) {
              if (rn) atomicAdd(hist_lds + rk, rn);
              rk = key; rn = 0u;
            }
            ++rn;
          }
        }
        const unsigned long long m = __ballot(valid && !sure);
        if (valid && !sure) {
          const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          queue[pos] = (unsigned short)(((mi * 16 + lr) << 6) | (ni * 16 + 4 * g + j));
        }
        cnt += __popcll(m);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (rn) atomicAdd(hist_lds + rk, rn);
  return cnt;
}

// re-score this wave's queued pairs exactly, 8 at a time, and bin them
__device__ __forceinline__ void verify_drain_queue(const unsigned short* queue, int cnt, int b_base, int n0, const float* __restrict__ A,
                                                   const float* __restrict__ B, const int32_t* __restrict__ lab_a,
                                                   const int32_t* __restrict__ lab_b, int D, const float* t_lds, unsigned* hist_lds,
                                                   int T, int lane) {
  constexpr int NB = 8;
  for (int q0 = 0; q0 < cnt; q0 += NB) {
    const float* pa[NB];
    const float* pb[NB];
    bool valid[NB], gen[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      valid[q] = q0 + q < cnt;
      const int e = queue[valid[q] ? q0 + q : q0];
      const int b = b_base + (e >> 6), n = n0 + (e & 63);
      pa[q] = A + (size_t)b * D; pb[q] = B + (size_t)n * D;
      gen[q] = lab_a[b] == lab_b[n];
    }
    double d2[NB];
    match_exact_d2_n<NB>(pa, pb, D, lane, d2);
    verify_bin_pairs<NB>(d2, valid, gen, t_lds, hist_lds, T, lane);
  }
}

// ------------------------------------------------------------------------------------------------
// Threshold search (frmap_match_radius[_packed], head_match.hip): every counted pair (i, j) of A x B (modes as the verification
// counts) with (float)sqrt(match_exact_d2) <= thresh is listed once as (i, j, dist); count[i] and total are exact whatever the
// capacity of the list.  NaN / inf distances are never accepted (thresh is finite).
// ------------------------------------------------------------------------------------------------
struct RadiusOut {
  int32_t* count;              // [P] accepted pairs per row of A (zeroed by radius_prep_kernel)
  unsigned long long* total;   // [1] accepted pairs = list slots reserved so far
  int32_t* pair;               // [capacity][2] = (i, j); null with capacity 0
  float* dist;                 // [capacity]
  long long capacity;
  float thresh;
};

// whether the labels let a pair through: 0 = all pairs, 1 = equal labels only, 2 = different labels only
__device__ __forceinline__ bool radius_filter_ok(int filter, int la, int lb) { return filter == 0 || (la == lb) == (filter == 1); }

// A wave collects its accepted pairs in its own LDS buffer (RADIUS_OB entries: (i, j) int2 [RADIUS_OB] | dist fp32 [RADIUS_OB]) and
// reserves list slots once per full buffer, not once per batch: a slot reservation is a returning atomic on ONE address for the whole
// device, and at 1 % of 134 M pairs accepted, one per 8-pair batch made the call 2.5x the time of the same GEMM without it.
constexpr int RADIUS_OB = 256;
constexpr int RADIUS_OB_BYTES = RADIUS_OB * 12;

// write out the wave's w buffered pairs: ONE atomic reserves their slots, then the lanes copy (i, j, dist) where the slot lies inside
// the list (whole lines: consecutive lanes, consecutive slots)
__device__ __forceinline__ void radius_flush(const RadiusOut& o, const int* obuf, int& w, int lane) {
  if (!w) return;                                  // (wave-uniform)
  unsigned long long base = 0ull;
  if (lane == 0) base = atomicAdd(o.total, (unsigned long long)w);
  base = __shfl(base, 0, 64);
  __builtin_amdgcn_wave_barrier();                 // (the buffer was written by other lanes of this wave)
  for (int e = lane; e < w; e += 64) {
    const long long slot = (long long)base + e;
    if (slot < o.capacity) {
      *(int2*)(o.pair + 2 * slot) = ((const int2*)obuf)[e];
      o.dist[slot] = ((const float*)(obuf + 2 * RADIUS_OB))[e];
    }
  }
  __builtin_amdgcn_wave_barrier();
  w = 0;
}

// NB pairs whose exact d2 every lane holds: lane q < NB takes pair q.  The accepted ones bump their row's count and join the wave's
// buffer (w entries so far, wave-uniform), which is flushed before it could overflow; the caller flushes what is left at its end.
template <int NB>
__device__ __forceinline__ void radius_emit(const double (&d2)[NB], const bool (&valid)[NB], const int (&pi)[NB], const int (&pj)[NB],
                                            const RadiusOut& o, int* obuf, int& w, int lane) {
  double d = 0.0;
  bool v = false;
  int i = 0, j = 0;
#pragma unroll
  for (int q = 0; q < NB; ++q)
    if (lane == q) { d = d2[q]; v = valid[q]; i = pi[q]; j = pj[q]; }
  const float dist = (float)sqrt(d);
  const bool hit = v && dist <= o.thresh;          // (NaN compares false)
  const unsigned long long m = __ballot(hit);
  if (!m) return;                                  // (wave-uniform)
  if (hit) {
    atomicAdd(o.count + i, 1);
    const int pos = w + __popcll(m & ((1ull << lane) - 1ull));
    ((int2*)obuf)[pos] = make_int2(i, j);
    ((float*)(obuf + 2 * RADIUS_OB))[pos] = dist;
  }
  w += __popcll(m);
  if (w > RADIUS_OB - NB) radius_flush(o, obuf, w, lane);
}

// Epilogue of conv1x1_pp_kernel<..., MATCH_JOIN>: bounds L <= d2 <= U as match_epilogue_hist.  With hi = the smallest fp32 >=
// next_up(thresh)^2, a pair with L > hi has (float)sqrt(d2) > thresh and is dropped at once, like a pair outside the problem, on or
// below the diagonal (self mode) or filtered out by its labels.  Every other pair - surely accepted or undecided: the list carries
// the exact distance, so both need the exact d2 - goes to this wave's LDS queue (the layout of match_epilogue_hist's: it holds the
// wave's whole 112 x 64 block).  A NaN bound is never > hi: such a pair is re-scored and rejected there.  Returns the queue length.
template <int MI>
__device__ __forceinline__ int match_epilogue_join(const f32x4_t (&acc)[MI][4], int b_base, int b_end, int n0, int G, int D, int M,
                                                   const float* __restrict__ stat_a, const float* __restrict__ stat_w,
                                                   const int32_t* __restrict__ lab_a, const int32_t* __restrict__ lab_b, int row0,
                                                   int filter, float hi, unsigned short* queue, int lane) {
  const int lr = lane & 15, g = lane >> 4;
  const float eps = 1e-6f, kf = (float)D, keps = kf * eps * eps, kap = match_kappa(3 * D);
  int cnt = 0;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int b = b_base + mi * 16 + lr;
    const f32x4_t sa = *(const f32x4_t*)(stat_a + 4 * (size_t)min(b, M - 1));
    const float a2 = sa[0], as = sa[1], ai = sa[2], ab = sa[3] + keps;
    const int la = filter ? lab_a[min(b, M - 1)] : 0;
    const int nmin = row0 >= 0 ? row0 + b + 1 : 0;   // self mode: only rows after the probe's own
    const float* sw_p = stat_w;                      // (opaque copies: see match_epilogue_hist)
    const int32_t* lb_p = lab_b;
    asm volatile("" : "+s"(sw_p), "+s"(lb_p));
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + ni * 16 + 4 * g + j;
        const f32x4_t sw = *(const f32x4_t*)(sw_p + 4 * (size_t)min(n, G - 1));
        const float d2 = a2 + sw[0] - 2.f * (acc[mi][ni][j] * ai * sw[2]) + 2.f * eps * (as - sw[1]) + keps;
        const float L = d2 - kap * (ab + sw[3]);
        bool keep = n < G && b < b_end && n >= nmin && !(L > hi);
        if (filter && keep) keep = radius_filter_ok(filter, la, lb_p[min(n, G - 1)]);
        const unsigned long long m = __ballot(keep);
        if (keep) {
          const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          queue[pos] = (unsigned short)(((mi * 16 + lr) << 6) | (ni * 16 + 4 * g + j));
        }
        cnt += __popcll(m);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return cnt;
}

// re-score this wave's queued pairs exactly, 8 at a time, and list the accepted ones
__device__ __forceinline__ void radius_drain_queue(const unsigned short* queue, int cnt, int b_base, int n0, const float* __restrict__ A,
                                                   const float* __restrict__ B, int D, const RadiusOut& o, int* obuf, int lane) {
  constexpr int NB = 8;
  int w = 0;
  for (int q0 = 0; q0 < cnt; q0 += NB) {
    const float* pa[NB];
    const float* pb[NB];
    bool valid[NB];
    int pi[NB], pj[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      valid[q] = q0 + q < cnt;
      const int e = queue[valid[q] ? q0 + q : q0];
      pi[q] = b_base + (e >> 6); pj[q] = n0 + (e & 63);
      pa[q] = A + (size_t)pi[q] * D; pb[q] = B + (size_t)pj[q] * D;
    }
    double d2[NB];
    match_exact_d2_n<NB>(pa, pb, D, lane, d2);
    radius_emit<NB>(d2, valid, pi, pj, o, obuf, w, lane);
  }
  radius_flush(o, obuf, w, lane);
}

// the epilogue of a match GEMM in mode MM (MATCH_TOP1: MatchRec records, MATCH_TOPR: MatchRecK records, same [slot][M] layout)
template <int MM, int MI>
__device__ __forceinline__ void match_epilogue(const f32x4_t (&acc)[MI][4], int b_base, int b_end, int n0, int G, int D, int M,
                                               const float* __restrict__ stat_a, const float* __restrict__ stat_w, void* recs,
                                               int lane) {
  if constexpr (MM == MATCH_TOP1)
    match_epilogue_records<MI>(acc, b_base, b_end, n0, G, D, M, stat_a, stat_w, (MatchRec*)recs, lane);
  else
    match_epilogue_topr<MI>(acc, b_base, b_end, n0, G, D, M, stat_a, stat_w, (MatchRecK*)recs, lane);
}

// ------------------------------------------------------------------------------------------------
// Shared conv epilogue.  After the K loop a lane holds, per 16x16 MFMA tile (mi, ni), 4 consecutive
// output channels (ni*16 + g*4 ..+3) of ONE pixel (mi*16 + lr).  Storing that directly is 8 bytes
// per lane scattered over 16 pixel rows per instruction (32-byte fragments of 128-byte lines).
// Instead each wave transposes 16 pixels at a time through its own LDS scratch (fp32, row pitch
// NI*64+16 bytes) so that 8 consecutive lanes own one pixel's channel run and every global access
// (residual load, output store) is 16 bytes per lane and a whole line per 8 (or 4) lanes.
//   v = acc + shift[c] (+ residual) ; activation (relu: 0 none, 1 ReLU, 2 GELU) ; round once to the storage dtype.
// Caller guarantees: all waves are past their last read of the LDS tiles (a barrier), `scratch`
// is this wave's private 16*(NI*64+16)-byte region, 16-byte aligned.
// ------------------------------------------------------------------------------------------------
// `rv_pre` (optional): the residual pieces already in registers, rv_pre[mi * PER_LANE + j] = the 16 bytes
// at (pixel m_wave0 + mi*16 + (j*64 + lane) / PARTS, channels co0 + ((j*64 + lane) % PARTS) * 8 ..+7);
// `res` is then only a flag (non-null = add them).
template <typename TT, int MI, int NI>
__device__ __forceinline__ void conv_epilogue(const f32x4_t (&acc)[MI][NI], char* scratch, int m_wave0, int M,
                                              int Cout, int co0, const float* __restrict__ shift,
                                              const typename TT::elem* __restrict__ res,
                                              typename TT::elem* __restrict__ out, int relu, int lane,
                                              const u32x4_t* rv_pre = nullptr) {
  constexpr int PITCH = NI * 64 + 16;      // bytes per pixel row in scratch
  constexpr int PARTS = NI * 2;            // 8-channel runs per pixel
  constexpr int PER_LANE = PARTS / 4;      // (16 px * PARTS) / 64 lanes
  const int lr = lane & 15, g = lane >> 4;
  // this lane's channel run is the same in every pass
  float sh[PER_LANE][8];
  int part[PER_LANE], prow[PER_LANE];
#pragma unroll
  for (int j = 0; j < PER_LANE; ++j) {
    const int idx = j * 64 + lane;
    prow[j] = idx / PARTS;
    part[j] = idx % PARTS;
    const f32x4_t s0 = *(const f32x4_t*)(shift + co0 + part[j] * 8), s1 = *(const f32x4_t*)(shift + co0 + part[j] * 8 + 4);
    sh[j][0] = s0[0]; sh[j][1] = s0[1]; sh[j][2] = s0[2]; sh[j][3] = s0[3];
    sh[j][4] = s1[0]; sh[j][5] = s1[1]; sh[j][6] = s1[2]; sh[j][7] = s1[3];
  }
  // residual: all of this lane's 16-byte pieces are requested up front (one global round trip,
  // not one per pass); they land while the LDS transposes run
  u32x4_t rv[MI][PER_LANE];
  if (res) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int j = 0; j < PER_LANE; ++j) {
        const int m = m_wave0 + mi * 16 + prow[j];
        rv[mi][j] = (u32x4_t){0u, 0u, 0u, 0u};
        if (rv_pre) rv[mi][j] = rv_pre[mi * PER_LANE + j];
        else if (m < M) rv[mi][j] = *(const u32x4_t*)(res + (size_t)m * Cout + co0 + part[j] * 8);
      }
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) *(f32x4_t*)(scratch + lr * PITCH + ni * 64 + g * 16) = acc[mi][ni];
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
      const f32x4_t a = *(const f32x4_t*)(scratch + prow[j] * PITCH + part[j] * 32);
      const f32x4_t b = *(const f32x4_t*)(scratch + prow[j] * PITCH + part[j] * 32 + 16);
      const int m = m_wave0 + mi * 16 + prow[j];
      if (m < M) {
        const size_t o = (size_t)m * Cout + co0 + part[j] * 8;
        float v[8] = {a[0] + sh[j][0], a[1] + sh[j][1], a[2] + sh[j][2], a[3] + sh[j][3],
                      b[0] + sh[j][4], b[1] + sh[j][5], b[2] + sh[j][6], b[3] + sh[j][7]};
        if (res) {
          float r[8];
          unpack8<TT>(rv[mi][j], r);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += r[e];
        }
        if (relu == 1) {
          // frmap_relu on two 4-vectors: written element by element the same instructions cost conv3x3_pp_kernel<.., MI = 7, RI>
          // one spilled register (csrc/build.sh's no-scratch check)
          f32x4_t lo4 = {v[0], v[1], v[2], v[3]}, hi4 = {v[4], v[5], v[6], v[7]};
          const f32x4_t z4 = {0.f, 0.f, 0.f, 0.f};
          lo4 = __builtin_elementwise_maximum(lo4, z4); hi4 = __builtin_elementwise_maximum(hi4, z4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[e] = lo4[e]; v[4 + e] = hi4[e]; }
        } else if (relu == 2) {  // exact (erf) GELU, nn.GELU() default
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752f));
        }
        *(u32x4_t*)(out + o) = pack8<TT>(v);
      }
    }
  }
}

// 2x2 / stride-2 max-pool fused into the epilogue (`self.pool(F.relu(self.bn(self.conv(x))))`, face_models.py:38-40,
// and SiameseNet's conv -> BN -> ReLU -> MaxPool2d(2) runs, :121-141).  The kernel enumerates its output pixels in
// POOL-MAJOR order - index m = 4 * window + (dy * 2 + dx) - so the 16 pixels of an MFMA column group are 4 whole
// pooling windows and a window's 4 pixels sit in 4 consecutive scratch rows: the pooled value is the max over those
// rows (max and the monotonic shift + ReLU commute: shift + act are applied once, after the max).  Writes pooled
// pixel (mp_wave0 + mi * 4 + window) as whole 16-byte runs like conv_epilogue.
template <typename TT, int MI, int NI>
__device__ __forceinline__ void conv_epilogue_pool2(const f32x4_t (&acc)[MI][NI], char* scratch, int mp_wave0, int MP,
                                                    int Cout, int co0, const float* __restrict__ shift,
                                                    typename TT::elem* __restrict__ out, int relu, int lane) {
  constexpr int PITCH = NI * 64 + 16, PARTS = NI * 2;
  const int lr = lane & 15, g = lane >> 4;
  // every lane reads (lanes >= 4 * PARTS redo windows 0..3 and store nothing): a lane that only ever wrote the scratch
  // would let the compiler drop all but its last write (its own view has no read in between) - seen in the ISA
  const bool active = lane < 4 * PARTS;
  const int win = (lane / PARTS) & 3, part = lane % PARTS;
  float sh[8];
  {
    const f32x4_t s0 = *(const f32x4_t*)(shift + co0 + part * 8), s1 = *(const f32x4_t*)(shift + co0 + part * 8 + 4);
    sh[0] = s0[0]; sh[1] = s0[1]; sh[2] = s0[2]; sh[3] = s0[3];
    sh[4] = s1[0]; sh[5] = s1[1]; sh[6] = s1[2]; sh[7] = s1[3];
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) *(f32x4_t*)(scratch + lr * PITCH + ni * 64 + g * 16) = acc[mi][ni];
    __builtin_amdgcn_wave_barrier();
    const char* src = scratch + (win * 4) * PITCH + part * 32;
    f32x4_t a = *(const f32x4_t*)src, b = *(const f32x4_t*)(src + 16);
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      const f32x4_t a2 = *(const f32x4_t*)(src + q * PITCH), b2 = *(const f32x4_t*)(src + q * PITCH + 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) { a[e] = frmap_max(a[e], a2[e]); b[e] = frmap_max(b[e], b2[e]); }
    }
    const int mp = mp_wave0 + mi * 4 + win;
    if (active && mp < MP) {
      float v[8] = {a[0] + sh[0], a[1] + sh[1], a[2] + sh[2], a[3] + sh[3], b[0] + sh[4], b[1] + sh[5], b[2] + sh[6], b[3] + sh[7]};
      if (relu == 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = frmap_relu(v[e]);
      }
      *(u32x4_t*)(out + (size_t)mp * Cout + co0 + part * 8) = pack8<TT>(v);
    }
  }
}

// split-K variant of the epilogue: the raw fp32 accumulator tile goes to this K-slice's slab
// ([M][Cout] fp32), transposed through LDS the same way so every store is 16 bytes per lane.
template <int MI, int NI>
__device__ __forceinline__ void conv_epilogue_partial(const f32x4_t (&acc)[MI][NI], char* scratch, int m_wave0, int M,
                                                      int Cout, int co0, float* __restrict__ slab, int lane) {
  constexpr int PITCH = NI * 64 + 16, PARTS = NI * 2, PER_LANE = PARTS / 4;
  const int lr = lane & 15, g = lane >> 4;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) *(f32x4_t*)(scratch + lr * PITCH + ni * 64 + g * 16) = acc[mi][ni];
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
      const int idx = j * 64 + lane, prow = idx / PARTS, part = idx % PARTS;
      const f32x4_t a = *(const f32x4_t*)(scratch + prow * PITCH + part * 32);
      const f32x4_t b = *(const f32x4_t*)(scratch + prow * PITCH + part * 32 + 16);
      const int m = m_wave0 + mi * 16 + prow;
      if (m < M) {
        float* o = slab + (size_t)m * Cout + co0 + part * 8;
        *(f32x4_t*)o = a;
        *(f32x4_t*)(o + 4) = b;
      }
    }
  }
}

// exact floor(n / d) for n, d < 65536 with magic = ceil(2^32 / d)
__host__ __device__ inline uint32_t frmap_magic(uint32_t d) {
  return (uint32_t)(((1ull << 32) + d - 1) / d);
}
__device__ __forceinline__ uint32_t fast_div(uint32_t n, uint32_t magic) { return __umulhi(n, magic); }

// exact floor(n / d) for 0 <= n < 2^31 and a run-time d >= 1 prepared on the host: a hardware-less integer division
// costs ~35 VALU instructions, this one a mul_hi and a shift.  d >= 2: k = ceil(log2 d), m = ceil(2^(31+k) / d) < 2^32,
// q = (n * m) >> (31 + k) = mul_hi(n, m) >> (k - 1)  (error term m*d - 2^(31+k) < d <= 2^k keeps it exact for n < 2^31).
struct FrmapDiv {
  uint32_t m;  // 0: d == 1
  uint32_t sh;
};
__host__ inline FrmapDiv frmap_div_make(uint32_t d) {
  FrmapDiv r = {0u, 0u};
  if (d <= 1) return r;
  uint32_t k = 0;
  while ((1ull << k) < d) ++k;
  r.m = (uint32_t)((((unsigned long long)1 << (31 + k)) + d - 1) / d);
  r.sh = k - 1;
  return r;
}
__device__ __forceinline__ int frmap_div(int n, FrmapDiv d) { return d.m ? (int)(__umulhi((uint32_t)n, d.m) >> d.sh) : n; }

// pool-major pixel order (conv_epilogue_pool2): m = 4 * w + q, window w = (n * Ho/2 + py) * Wo/2 + px row-major over the
// POOLED map, q = dy * 2 + dx inside the 2x2 window  ->  output pixel (n, 2 py + dy, 2 px + dx)
struct FrmapPoolOrder {
  FrmapDiv dWin, dWo2;  // divisions by (Ho/2 * Wo/2) and Wo/2
  int Win, Wo2;
};
__device__ __forceinline__ void frmap_pool_coords(int m, const FrmapPoolOrder& o, int& n, int& oy, int& ox) {
  const int w = m >> 2, q = m & 3;
  n = frmap_div(w, o.dWin);
  const int rem = w - n * o.Win;
  const int py = frmap_div(rem, o.dWo2);
  oy = 2 * py + (q >> 1);
  ox = 2 * (rem - py * o.Wo2) + (q & 1);
}

// host-side error plumbing
void frmap_set_error(const char* fmt, ...);
// raise a kernel's dynamic-LDS limit on the CURRENT device (once per (kernel, device)); 0 or -2 with the error set
int frmap_big_lds(const void* kern, int bytes);
// second-generation fused ResNet stem (stem_s2d.hip): 1 = launched, 0 = shape not taken, < 0 = error
int frmap_stem_s2d(const float* x_nchw, const unsigned char* x_u8, const float* mean3, const float* std3, const void* w_packed_c3,
                   const float* shift, void* out, int B, int Hi, int Wi, int dtype, hipStream_t st);
int frmap_batch_invariant();   // 1: planners must not look at the batch size (c_api.cpp)
int frmap_cu_count();          // compute units of the current device (asked once; 256 where the runtime cannot say)
// the conv planner (conv_plan.h) with this process's tuning, CU count and batch-invariant flag (conv_igemm.hip)
ConvPlan frmap_conv_plan(const ConvLayer& L);
// launches a layer the planner gave to the second generation (conv_pp.hip: CK_PP, CK_PP_S2, CK_PP_1X1); 0 or an error
int frmap_conv_pp_launch(const ConvLayer& L, const ConvPlan& q, const void* in, const void* w_packed, const float* shift,
                         const void* residual, void* out, const void* ds_in, const void* ds_w, int relu, int dtype, hipStream_t st);
// what the verification counts' match GEMM (MATCH_HIST) takes besides the operands:
// tab: t [T] | lo [T] | hi [T] (fp32, device); hist: u64 [2][T + 1] accumulated into; rescored: u64 += pairs re-scored exactly
struct FrmapVerifyGemm {
  const float* A;           // fp32 [P][D]
  const float* B;           // fp32 [Q][D]
  const int32_t* lab_a;
  const int32_t* lab_b;
  const float* tab;
  unsigned long long* hist;
  unsigned long long* rescored;
  int row0;                 // -1: cross mode; else A = rows [row0, row0 + P) of B, pairs with row0 + i < j
  int T;
};
// what the threshold search's match GEMM (MATCH_JOIN) takes besides the operands
struct FrmapRadiusGemm {
  const float* A;           // fp32 [P][D]
  const float* B;           // fp32 [Q][D]
  const int32_t* lab_a;     // may be null when filter == 0
  const int32_t* lab_b;
  RadiusOut out;
  unsigned long long* rescored;   // u64 += pairs re-scored exactly
  float hi;                 // the smallest fp32 >= next_up(thresh)^2
  int row0;                 // as FrmapVerifyGemm
  int filter;               // 0 = all pairs, 1 = equal labels only, 2 = different labels only
};
// The split-fp16 match GEMM (conv1x1_pp_kernel<F16, ..., mode>, conv_pp.hip) of P probes against a packed gallery of G rows:
// mode MATCH_TOP1 / MATCH_TOPR writes MatchRec / MatchRecK records to `out` ([Gpad / 64][P]); MATCH_HIST takes a FrmapVerifyGemm*
// as `out`, MATCH_JOIN a FrmapRadiusGemm*.  1 = launched, 0 = shape not taken (nothing launched), < 0 = error; probes3 == nullptr: plan only.
int frmap_match_gemm(int mode, const void* probes3, const void* gallery_packed, const float* stat_a, const float* stat_w, void* out,
                     int P, int G, int D, hipStream_t st);
// label_out[0 .. n) = -1 (frmap_match_topk's k = 1 entry-mode outputs; head_match.hip)
int frmap_match_topk_fill_labels(int32_t* label_out, int n, hipStream_t st);
#define FRMAP_REQUIRE(cond, ...)        \
  do {                                  \
    if (!(cond)) {                      \
      frmap_set_error(__VA_ARGS__);     \
      return -1;                        \
    }                                   \
  } while (0)
#define FRMAP_LAUNCH_CHECK()                                           \
  do {                                                                 \
    hipError_t e__ = hipGetLastError();                                \
    if (e__ != hipSuccess) {                                           \
      frmap_set_error("launch failed: %s", hipGetErrorString(e__));    \
      return -2;                                                       \
    }                                                                  \
  } while (0)
