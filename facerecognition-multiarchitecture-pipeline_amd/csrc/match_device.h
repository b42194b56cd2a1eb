// The gallery matcher's device code and the host interface between its two translation units: head_match.hip (entry points, exact
// scans, finalize kernels) and conv_pp.hip (the split-fp16 match GEMM, conv1x1_pp_kernel<F16, ..., MM>).  Nothing else includes it.
#pragma once
#include "frmap_common.h"

// ------------------------------------------------------------------------------------------------
// Top-1 gallery match (the reference's compare_faces loop, app.py:58-63) behind a GEMM: candidate records.
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
// d2e from the two rows' (sum x^2, sum x), their dot product and keps = K eps^2: THE statement of the expression, in the operation
// order every record, bin and re-scored count depends on
__device__ __forceinline__ float match_expanded_d2(float a2, float as, float w2, float ws, float dot, float keps) {
  const float eps = 1e-6f;
  const float d2 = a2 + w2 - 2.f * dot + 2.f * eps * (as - ws) + keps;
  return d2;
}
// A pair WITHOUT a bound.  The expanded form says nothing once it leaves fp32: a row whose squared norm overflows (norm above about
// 1.8e19) has sum x^2 = band = +inf, so d2 and delta are +inf and L = inf - inf is NaN; two norms that are finite but whose sum is
// not give d2 = U = +inf with a finite delta, a "lower bound" of +inf above an exact distance that is finite; a row with a NaN
// or an infinity in it gives NaN.  The exact distance of the first two kinds is finite (fp32 differences, squares summed in float64),
// and the documented answer lists them.  U = d2 + delta is finite only if d2 and delta both are, and then so is L: whenever U is not
// finite the pair's bounds become (-inf, +inf), the honest ones.  Every epilogue then treats it as in band and the exact re-score
// decides: a record lists it first (lo = -inf <= every tau, up = +inf never lowers a tau), the verification counts queue it
// (not sure), the threshold search keeps it (-inf is not > hi).  No NaN ever reaches a record, an fminf chain or a compare.
__device__ __forceinline__ void match_unbounded(float& L, float& U) {
  if (!__builtin_isfinite(U)) { L = -INFINITY; U = INFINITY; }
}

enum MatchMode { MATCH_NONE = 0, MATCH_TOP1 = 1, MATCH_TOPR = 2, MATCH_HIST = 3, MATCH_JOIN = 4 };   // MATCH_HIST: verification counts, MATCH_JOIN: threshold search

// What a wave of the split-fp16 match GEMM holds after the K loop: lane (lr, g) has, per MFMA tile (mi, ni), the scaled dot
// products of probe b_base + mi * 16 + lr with gallery rows n0 + ni * 16 + 4 g + j.  Probes end at b_end (<= M, the probe count),
// the gallery at G rows of width D.  Row statistics (match_row_prep_kernel): (sum x^2, sum x, 1 / row scale, band(x)).
struct MatchTile {
  int b_base, b_end, n0, G, D, M;
  const float* __restrict__ stat_a;
  const float* __restrict__ stat_w;
};

// The bound walk of the four match epilogues over a wave's MI*16 x 64 block, one probe row (mi) at a time:
//   row_begin(b) -> the pointer this row's gallery statistics are read through (stat_w, or an opaque copy of it: match_epilogue_hist)
//   pair(b, n, code, L, U): L <= exact d2 <= U of probe b and gallery row n, (-inf, +inf) where the expanded form has no finite
//                           bound (match_unbounded), never NaN; code = the pair's place in the block as the queues
//                           hold it, (probe row << 6) | gallery row.  b and n may lie past the problem (their loads are clamped).
//   row_end(b)
// The gallery-row statistics are re-read per (mi, ni) block (L1 hits) instead of being held for the whole epilogue, so the live set
// stays at acc + ~30 registers: the kernels around an epilogue count their LDS-DMA with s_waitcnt vmcnt(n) and must not spill
// (csrc/build.sh checks).
template <int MI, typename RowBegin, typename Pair, typename RowEnd>
__device__ __forceinline__ void match_walk(const f32x4_t (&acc)[MI][4], const MatchTile& t, int lane, RowBegin&& row_begin,
                                           Pair&& pair, RowEnd&& row_end) {
  const int lr = lane & 15, g = lane >> 4;
  const float eps = 1e-6f, kf = (float)t.D, keps = kf * eps * eps, kap = match_kappa(3 * t.D);
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int b = t.b_base + mi * 16 + lr;
    const f32x4_t sa = *(const f32x4_t*)(t.stat_a + 4 * (size_t)min(b, t.M - 1));
    const float a2 = sa[0], as = sa[1], ai = sa[2], ab = sa[3] + keps;
    const float* sw_p = row_begin(b);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = t.n0 + ni * 16 + 4 * g + j;
        const f32x4_t sw = *(const f32x4_t*)(sw_p + 4 * (size_t)min(n, t.G - 1));
        const float d2 = match_expanded_d2(a2, as, sw[0], sw[1], acc[mi][ni][j] * ai * sw[2], keps);
        const float dl = kap * (ab + sw[3]);
        float L = d2 - dl, U = d2 + dl;
        match_unbounded(L, U);
        pair(b, n, ((mi * 16 + lr) << 6) | (ni * 16 + 4 * g + j), L, U);
      }
    }
    row_end(b);
    __builtin_amdgcn_sched_barrier(0);   // one probe row's loads at a time: no hoisting of the next row's statistics loads
  }
}

// MATCH_TOP1 (conv1x1_pp_kernel<.., MATCH_TOP1>): the wave's 64 gallery rows are one slot (n0 / 64); records are laid out [slot][M].
// Rows past G are +inf: never candidates.
template <int MI>
__device__ __forceinline__ void match_epilogue_records(const f32x4_t (&acc)[MI][4], const MatchTile& t, MatchRec* __restrict__ recs,
                                                       int lane) {
  MatchRec* out = recs + (size_t)(t.n0 >> 6) * t.M;
  float l1, l2, up;
  int i1;
  match_walk<MI>(
      acc, t, lane,
      [&](int) {
        l1 = INFINITY; l2 = INFINITY; up = INFINITY; i1 = -1;
        return t.stat_w;
      },
      [&](int, int n, int, float L, float U) {
        if (n >= t.G) { L = INFINITY; U = INFINITY; }
        if (L < l1) { l2 = l1; l1 = L; i1 = n; }   // rows ascend inside the lane: the first of equal L keeps the index,
        else if (L < l2) l2 = L;                   // the second lands in lo2 (= lo1: the whole slot is re-scored)
        up = fminf(up, U);
      },
      [&](int b) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const float ol1 = __shfl_xor(l1, o, 64), ol2 = __shfl_xor(l2, o, 64), ou = __shfl_xor(up, o, 64);
          const int oi1 = __shfl_xor(i1, o, 64);
          const float nl2 = fminf(fminf(l2, ol2), fmaxf(l1, ol1));
          if (ol1 < l1) { l1 = ol1; i1 = oi1; }
          l2 = nl2; up = fminf(up, ou);
        }
        if (lane < 16 && b < t.b_end) {
          MatchRec r; r.lo1 = l1; r.idx = i1; r.lo2 = l2; r.up = up;
          out[b] = r;
        }
      });
}

// ------------------------------------------------------------------------------------------------
// Top-k gallery search behind the same GEMM: per probe and 64-row slot, the R = 4 smallest lower bounds L of the slot (ascending,
// first row first among equal L) with their rows and upper bounds U, and `rest` = the (R+1)-th smallest L, a lower bound on every
// row of the slot that is not listed.  Error bounds as above.  match_topk_finalize_kernel (head_match.hip) takes
// tau = the k-th smallest listed U (per distinct label in identity mode) and re-scores exactly every listed row with L <= tau and
// every row of a slot whose rest <= tau.  An identity enrolled up to R times in one slot never forces a whole-slot re-score.
// ------------------------------------------------------------------------------------------------
constexpr int MATCH_R = 4;
struct __attribute__((aligned(16))) MatchRecK {   // 64 bytes
  float lo[MATCH_R];
  int idx[MATCH_R];   // -1: none
  float up[MATCH_R];
  float rest;
  int pad[3];
};

// insert (L, n, U) into an ascending R-list; what falls off (or L itself) lowers `rest`.  Strict compares: an equal L goes after,
// and L is never NaN (match_unbounded): a pair without a bound comes as (-inf, +inf), is listed ahead of every bounded one and, once
// the list is full of its kind, pulls `rest` down to -inf, so the finalize re-scores the whole slot.
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

// MATCH_TOPR: MatchRecK records, the [slot][M] layout of match_epilogue_records
template <int MI>
__device__ __forceinline__ void match_epilogue_topr(const f32x4_t (&acc)[MI][4], const MatchTile& t, MatchRecK* __restrict__ recs,
                                                    int lane) {
  MatchRecK* out = recs + (size_t)(t.n0 >> 6) * t.M;
  float lo[MATCH_R], up[MATCH_R], rest;
  int ix[MATCH_R];
  match_walk<MI>(
      acc, t, lane,
      [&](int) {
        rest = INFINITY;
#pragma unroll
        for (int j = 0; j < MATCH_R; ++j) { lo[j] = INFINITY; up[j] = INFINITY; ix[j] = -1; }
        return t.stat_w;
      },
      [&](int, int n, int, float L, float U) {
        if (n >= t.G) { L = INFINITY; U = INFINITY; }
        match_topr_insert(lo, ix, up, rest, L, n, U);   // rows ascend inside the lane
      },
      [&](int b) {
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
        if (lane < 16 && b < t.b_end) {
          MatchRecK r;
#pragma unroll
          for (int j = 0; j < MATCH_R; ++j) { r.lo[j] = lo[j]; r.idx[j] = ix[j]; r.up[j] = up[j]; }
          r.rest = rest; r.pad[0] = r.pad[1] = r.pad[2] = 0;
          out[b] = r;
        }
      });
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
// The pair feed of the verification counts and the threshold search: PAIR_NB pairs (i = row of A, j = row of B) that a wave scores
// exactly in one go, formed either from a VS_PB x VS_QB block of A x B (the exact scans) or from a match-GEMM wave's queue, and
// handed with their exact d2 to a sink (VerifySink bins them, RadiusSink lists the accepted ones).
// ------------------------------------------------------------------------------------------------
constexpr int PAIR_NB = 8;
constexpr int VS_PB = 8, VS_QB = 512;   // one workgroup of an exact scan = VS_PB rows of A x VS_QB rows of B
struct PairBatch {
  int i[PAIR_NB], j[PAIR_NB];   // always rows inside A and B (clamped / repeated for the pairs that are not valid)
  bool valid[PAIR_NB];
};

// self mode (row0 >= 0: A = rows [row0, row0 + P) of B, pairs with row0 + i < j): block (i0, j0) has nothing above the diagonal
__device__ __forceinline__ bool pair_block_below_diagonal(int i0, int j0, int Q, int row0) {
  return row0 >= 0 && min(j0 + VS_QB, Q) - 1 <= row0 + i0;
}
// pairs base .. base + PAIR_NB - 1 (row-major) of the block at (i0, j0); a pair counts when it lies inside the problem, above the
// diagonal in self mode, and sink.want(i, j).  False when none of them counts (wave-uniform).
template <typename Sink>
__device__ __forceinline__ bool pair_batch_from_block(PairBatch& pb, int base, int i0, int j0, int P, int Q, int row0,
                                                      const Sink& sink) {
  bool any = false;
#pragma unroll
  for (int q = 0; q < PAIR_NB; ++q) {
    const int i = i0 + (base + q) / VS_QB, j = j0 + (base + q) % VS_QB;
    pb.i[q] = min(i, P - 1); pb.j[q] = min(j, Q - 1);
    pb.valid[q] = i < P && j < Q && (row0 < 0 || row0 + i < j) && sink.want(pb.i[q], pb.j[q]);
    any |= pb.valid[q];
  }
  return any;
}
// entries q0 .. q0 + PAIR_NB - 1 of a match-GEMM wave's queue of `cnt` u16 codes (match_walk's: (probe row << 6) | gallery row of the
// wave's block at (b_base, n0)); entries past the end repeat entry q0
__device__ __forceinline__ void pair_batch_from_queue(PairBatch& pb, const unsigned short* queue, int q0, int cnt, int b_base, int n0) {
#pragma unroll
  for (int q = 0; q < PAIR_NB; ++q) {
    pb.valid[q] = q0 + q < cnt;
    const int e = queue[pb.valid[q] ? q0 + q : q0];
    pb.i[q] = b_base + (e >> 6); pb.j[q] = n0 + (e & 63);
  }
}
template <typename Sink>
__device__ __forceinline__ void pair_batch_score(const PairBatch& pb, const float* __restrict__ A, const float* __restrict__ B, int D,
                                                 int lane, Sink& sink) {
  const float* pa[PAIR_NB];
  const float* pg[PAIR_NB];
#pragma unroll
  for (int q = 0; q < PAIR_NB; ++q) { pa[q] = A + (size_t)pb.i[q] * D; pg[q] = B + (size_t)pb.j[q] * D; }
  double d2[PAIR_NB];
  match_exact_d2_n<PAIR_NB>(pa, pg, D, lane, d2);
  sink.take(pb, d2, lane);
}
// an exact scan's workgroup (4 waves): every pair of block (blockIdx.x, blockIdx.y) that counts, PAIR_NB at a time per wave
template <typename Sink>
__device__ __forceinline__ void pair_scan_block(const float* __restrict__ A, const float* __restrict__ B, int P, int Q, int D, int row0,
                                                Sink& sink) {
  const int i0 = blockIdx.x * VS_PB, j0 = blockIdx.y * VS_QB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int base = wave * PAIR_NB; base < VS_PB * VS_QB; base += 4 * PAIR_NB) {
    PairBatch pb;
    if (!pair_batch_from_block(pb, base, i0, j0, P, Q, row0, sink)) continue;   // (wave-uniform)
    pair_batch_score(pb, A, B, D, lane, sink);
  }
}
// a match-GEMM wave re-scores its queued pairs exactly
template <typename Sink>
__device__ __forceinline__ void pair_drain_queue(const unsigned short* queue, int cnt, int b_base, int n0, const float* __restrict__ A,
                                                 const float* __restrict__ B, int D, int lane, Sink& sink) {
  for (int q0 = 0; q0 < cnt; q0 += PAIR_NB) {
    PairBatch pb;
    pair_batch_from_queue(pb, queue, q0, cnt, b_base, n0);
    pair_batch_score(pb, A, B, D, lane, sink);
  }
}
// append the pairs of the lanes that say `push` to the wave's queue of `cnt` codes (cnt stays wave-uniform)
__device__ __forceinline__ void pair_queue_push(unsigned short* queue, int& cnt, bool push, int code) {
  const unsigned long long m = __ballot(push);
  if (push) {
    const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    queue[pos] = (unsigned short)code;
  }
  cnt += __popcll(m);
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

// bins the pairs of a batch in the workgroup's LDS histogram: lane q < PAIR_NB takes pair q
struct VerifySink {
  const int32_t* __restrict__ lab_a;
  const int32_t* __restrict__ lab_b;
  const float* t_lds;
  unsigned* hist_lds;
  int T;
  __device__ __forceinline__ bool want(int, int) const { return true; }
  __device__ __forceinline__ void take(const PairBatch& pb, const double (&d2)[PAIR_NB], int lane) {
    double d = 0.0;
    bool v = false;
    int i = 0, j = 0;
#pragma unroll
    for (int q = 0; q < PAIR_NB; ++q)
      if (lane == q) { d = d2[q]; v = pb.valid[q]; i = pb.i[q]; j = pb.j[q]; }
    if (v) {
      const float dist = (float)sqrt(d);
      atomicAdd(hist_lds + (lab_a[i] == lab_b[j] ? 0 : T + 1) + verify_bin(t_lds, T, dist), 1u);
    }
  }
};

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

// Epilogue of conv1x1_pp_kernel<..., MATCH_HIST>: pair (probe b = A row, gallery row n = B row) has L <= d2 <= U.  With the host's
// brackets (d2 <= lo_k => dist <= t_k, d2 > hi_k => dist > t_k, both ascending) the pair's bin is certain when kU = the first k with
// U <= lo_k has L > hi_{kU - 1} (or kU = 0) - which no pair without a bound, (-inf, +inf), ever has: then d2 <= lo_kU and d2 > hi_k for every k < kU.  Certain pairs are
// binned at once; the others go to this wave's LDS queue and are re-scored by pair_drain_queue.  Returns the queue length (wave-uniform).
template <int MI>
__device__ __forceinline__ int match_epilogue_hist(const f32x4_t (&acc)[MI][4], const MatchTile& t, const FrmapVerifyGemm& v,
                                                   const float* lo_lds, const float* hi_lds, unsigned* hist_lds,
                                                   unsigned short* queue, int lane) {
  const int T = v.T;
  int cnt = 0;
  // a lane's certain pairs mostly land in the same bin as the one before (every lane of the wave, often in the same bin): runs
  // are merged in registers and added with one LDS atomic per run instead of one per pair (64-way serialised on a shared bin)
  int rk = 0;
  unsigned rn = 0u;
  int la, nmin;
  const int32_t* lb_p;
  match_walk<MI>(
      acc, t, lane,
      [&](int b) {
        la = v.lab_a[min(b, t.M - 1)];
        nmin = v.row0 >= 0 ? v.row0 + b + 1 : 0;   // self mode: only rows after the probe's own
        // re-read the gallery rows' statistics and labels per probe row: opaque copies of the pointers keep the compiler from merging
        // the 16 rows' loads of all MI probe rows into one set held across the whole epilogue (~80 registers next to acc)
        const float* sw_p = t.stat_w;
        lb_p = v.lab_b;
        asm volatile("" : "+s"(sw_p), "+s"(lb_p));
        return sw_p;
      },
      [&](int b, int n, int code, float L, float U) {
        const bool valid = n < t.G && b < t.b_end && n >= nmin;
        bool sure = false;
        if (valid) {
          const int k = verify_bin(lo_lds, T, U);
          // (a pair without a bound is never sure: its U = +inf is above every lo_k, so k = T >= 1, and its L = -inf is not > hi_{T-1})
          sure = k == 0 || L > hi_lds[k - 1];
          if (sure) {
            const int key = (la == lb_p[min(n, t.G - 1)] ? 0 : T + 1) + k;
            if (key != rk) {
              if (rn) atomicAdd(hist_lds + rk, rn);
              rk = key; rn = 0u;
            }
            ++rn;
          }
        }
        pair_queue_push(queue, cnt, valid && !sure, code);
      },
      [](int) {});
  if (rn) atomicAdd(hist_lds + rk, rn);
  return cnt;
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

// lists the accepted pairs of a batch; the labels (exact scans only: the GEMM's epilogue filters before it queues) decide which
// pairs of a block count at all
struct RadiusSink {
  RadiusOut o;
  int* obuf;                   // this wave's LDS buffer
  const int32_t* __restrict__ lab_a;
  const int32_t* __restrict__ lab_b;
  int filter;
  int w;                       // buffered pairs (wave-uniform)
  __device__ __forceinline__ bool want(int i, int j) const { return !filter || radius_filter_ok(filter, lab_a[i], lab_b[j]); }
  // write out the wave's w buffered pairs: ONE atomic reserves their slots, then the lanes copy (i, j, dist) where the slot lies
  // inside the list (whole lines: consecutive lanes, consecutive slots).  Every user calls it once more at its end.
  __device__ __forceinline__ void flush(int lane) {
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
  // lane q < PAIR_NB takes pair q.  The accepted ones bump their row's count and join the wave's buffer, which is flushed before it
  // could overflow.
  __device__ __forceinline__ void take(const PairBatch& pb, const double (&d2)[PAIR_NB], int lane) {
    double d = 0.0;
    bool v = false;
    int i = 0, j = 0;
#pragma unroll
    for (int q = 0; q < PAIR_NB; ++q)
      if (lane == q) { d = d2[q]; v = pb.valid[q]; i = pb.i[q]; j = pb.j[q]; }
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
    if (w > RADIUS_OB - PAIR_NB) flush(lane);
  }
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

// Epilogue of conv1x1_pp_kernel<..., MATCH_JOIN>: a pair with L > hi has (float)sqrt(d2) > thresh and is dropped at once, like a
// pair outside the problem, on or below the diagonal (self mode) or filtered out by its labels.  Every other pair - surely accepted
// or undecided: the list carries the exact distance, so both need the exact d2 - goes to this wave's LDS queue (the layout of
// match_epilogue_hist's: it holds the wave's whole 112 x 64 block).  A pair without a bound (L = -inf) is never > hi: it is re-scored
// and accepted or rejected there on its exact distance.  Returns the queue length.
template <int MI>
__device__ __forceinline__ int match_epilogue_join(const f32x4_t (&acc)[MI][4], const MatchTile& t, const FrmapRadiusGemm& r,
                                                   unsigned short* queue, int lane) {
  int cnt = 0;
  int la, nmin;
  const int32_t* lb_p;
  match_walk<MI>(
      acc, t, lane,
      [&](int b) {
        la = r.filter ? r.lab_a[min(b, t.M - 1)] : 0;
        nmin = r.row0 >= 0 ? r.row0 + b + 1 : 0;     // self mode: only rows after the probe's own
        const float* sw_p = t.stat_w;                // (opaque copies: see match_epilogue_hist)
        lb_p = r.lab_b;
        asm volatile("" : "+s"(sw_p), "+s"(lb_p));
        return sw_p;
      },
      [&](int b, int n, int code, float L, float) {
        bool keep = n < t.G && b < t.b_end && n >= nmin && !(L > r.hi);
        if (r.filter && keep) keep = radius_filter_ok(r.filter, la, lb_p[min(n, t.G - 1)]);
        pair_queue_push(queue, cnt, keep, code);
      },
      [](int) {});
  return cnt;
}

// ------------------------------------------------------------------------------------------------
// The split-fp16 match GEMM (conv1x1_pp_kernel<F16, ..., mode>, conv_pp.hip) of P probes against a packed gallery of G rows.
// ------------------------------------------------------------------------------------------------
struct FrmapMatchGemm {
  const void* probes3;          // fp16 [P][3 D] rows (a_hi | a_hi | a_lo), match_row_prep_kernel
  const void* gallery_packed;   // frmap_match_pack_gallery
  const float* stat_a;          // [P][4]
  const float* stat_w;          // [G][4]
  int P, G, D;
};
// whether the GEMM takes the shape (T: the verification counts' thresholds); if not, the caller answers from its exact scan
bool frmap_match_gemm_takes(int P, int G, int D, int T = 1);
// one launch each, of a shape the GEMM takes; 0 or an error.  Records: [Gpad / 64][P], Gpad = G rounded up to 256.
int frmap_match_gemm_records(const FrmapMatchGemm& g, MatchRec* recs, hipStream_t st);    // MATCH_TOP1
int frmap_match_gemm_records(const FrmapMatchGemm& g, MatchRecK* recs, hipStream_t st);   // MATCH_TOPR
int frmap_match_gemm_hist(const FrmapMatchGemm& g, const FrmapVerifyGemm& v, hipStream_t st);
int frmap_match_gemm_join(const FrmapMatchGemm& g, const FrmapRadiusGemm& r, hipStream_t st);
// label_out[0 .. n) = -1 (frmap_match_topk's k = 1 entry-mode outputs; head_match.hip)
int frmap_match_topk_fill_labels(int32_t* label_out, int n, hipStream_t st);
