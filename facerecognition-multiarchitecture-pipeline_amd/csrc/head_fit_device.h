// The device code that the head-fitting translation units share (head_fit.hip: the linear step and its groups; head_fit_hidden.hip:
// the hidden-layer step; head_fit_pair.hip: the pair step; head_fit_margin.hip: the margin step; head_fit_embed.hip: the embedding step): the tile walk of both GEMMs, its operand loaders and the bodies of the three
// kernels.  The kernels themselves (`__global__`) stay with their launchers: a code object holds the kernels of ONE of the files, so
// adding a kernel to one file leaves the other files' code objects - LDS layout, register allocation, instructions - as they are.
#pragma once
#include "frmap_common.h"
#include "head_fit_rule.h"
#include "head_fit_twin.h"

constexpr int HF_T = 32;                      // tile edge
constexpr int HF_KS = 32;                     // k of one staging step (four steps a chain)
constexpr int HF_PITCH = HF_KS + 1;
constexpr int HF_WAVES = 4;
constexpr int HF_SOFTMAX_MAX_BLOCKS = 2048;
static_assert(FRMAP_HEAD_FIT_CHAIN % HF_KS == 0 && HF_KS % 2 == 0, "a chain is whole staging steps of whole MFMA steps");

__device__ __forceinline__ void hf_add(uint64_t* p, uint64_t v) {
  __hip_atomic_fetch_add((unsigned long long*)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct HfSmem {
  float stage[HF_WAVES][2][HF_T * HF_PITCH];
  float part[HF_WAVES][HF_T * HF_T];
};

// The chains of one output tile: tot[q] of thread tid is element (i, j) = ((tid >> 5) + 8 q, tid & 31) of the tile, the sum over
// the chains of K in ascending order.  `op.load(k0, K, li, lk, a, b)` fetches this lane's 16 + 16 operand values of one staging
// step - element `it` of an operand is (tile row, k) = (2 it + lk, k0 + li) where its flag (A_K_FAST for a, B_K_FAST for b) says
// that k is contiguous in memory, else (li, k0 + 2 it + lk) - with +0 outside the problem.  A loader issues all of its loads from
// clamped, always valid addresses before it looks at any of them: a load per branch would cost a memory round trip each.
template <bool A_K_FAST, bool B_K_FAST, class OP>
__device__ __forceinline__ void hf_tile_chains(HfSmem& sm, int K, bool ragged, int vi, int vj, const OP& op, float (&tot)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lk = lane >> 5;
  float* As = sm.stage[wave][0];
  float* Bs = sm.stage[wave][1];
#pragma unroll
  for (int q = 0; q < 4; ++q) tot[q] = 0.0f;
  const int chains = (K + FRMAP_HEAD_FIT_CHAIN - 1) / FRMAP_HEAD_FIT_CHAIN;
  for (int j0 = 0; j0 < chains; j0 += HF_WAVES) {                 // (uniform over the workgroup: every barrier is reached by all)
    const int chain = j0 + wave;
    const bool live = chain < chains;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int sub = 0; sub < FRMAP_HEAD_FIT_CHAIN / HF_KS; ++sub) {
      const int k0 = chain * FRMAP_HEAD_FIT_CHAIN + sub * HF_KS;
      __syncthreads();                                            // the staging tiles are free again
      if (live && k0 < K) {
        float a[16], b[16];
        op.load(k0, K, li, lk, a, b);
#pragma unroll
        for (int it = 0; it < 16; ++it) {
          const int row = A_K_FAST ? it * 2 + lk : li, kk = A_K_FAST ? li : it * 2 + lk;
          const int rowb = B_K_FAST ? it * 2 + lk : li, kkb = B_K_FAST ? li : it * 2 + lk;
          As[row * HF_PITCH + kk] = a[it];
          Bs[rowb * HF_PITCH + kkb] = b[it];
        }
      }
      __syncthreads();
      if (live && k0 < K) {
        if (!ragged) {
#pragma unroll
          for (int kk = 0; kk < HF_KS; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[li * HF_PITCH + kk + lk], Bs[li * HF_PITCH + kk + lk], acc, 0, 0, 0);
        } else {
          // lane (li, lk) owns elements (i, j) = (2 q + lk, li), q = 0 .. 15
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int i = 2 * q + lk;
            if (i < vi && li < vj) {
              float c = acc[q];
#pragma unroll 8
              for (int kk = 0; kk < HF_KS; ++kk) c = fmaf(As[i * HF_PITCH + kk], Bs[li * HF_PITCH + kk], c);
              acc[q] = c;
            }
          }
        }
      }
    }
    // the partial tile of this chain, row-major
    if (live) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = ragged ? 2 * r + lk : (r & 3) + 8 * (r >> 2) + 4 * lk;
        sm.part[wave][i * HF_T + li] = acc[r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int wv = 0; wv < HF_WAVES; ++wv) {
      if (j0 + wv < chains) {
#pragma unroll
        for (int q = 0; q < 4; ++q) tot[q] = tot[q] + sm.part[wv][tid + 256 * q];
      }
    }
  }
}

// the operands of the logits tile (b0, c0): A = x' of the batch rows (K_FAST: k is contiguous in x and in w), B = w
struct HfLogitsOp {
  const float* x;
  const uint8_t* keep;
  const float* w;
  const int* s_src;      // LDS: the row of x behind tile row i, or -1
  int* s_bad;            // LDS: set where a staged feature of tile row i is non-finite
  float keep_scale;
  int b0, c0, B, D, C;
  __device__ __forceinline__ void load(int k0, int K, int li, int lk, float (&a)[16], float (&b)[16]) const {
    const int k = k0 + li;
    const bool kin = k < K;
    const size_t kc = (size_t)(kin ? k : K - 1);
    int src[16];
    float xv[16], wv[16];
    int kb[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) src[it] = s_src[it * 2 + lk];
#pragma unroll
    for (int it = 0; it < 16; ++it) xv[it] = x[(size_t)(src[it] < 0 ? 0 : src[it]) * (size_t)D + kc];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int c = c0 + it * 2 + lk;
      wv[it] = w[(size_t)(c < C ? c : C - 1) * (size_t)D + kc];
    }
    if (keep) {                                                   // (uniform)
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        const int bi = b0 + it * 2 + lk;
        kb[it] = (int)keep[(size_t)(bi < B ? bi : B - 1) * (size_t)D + kc];
      }
    } else {
#pragma unroll
      for (int it = 0; it < 16; ++it) kb[it] = -1;
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const bool valid = kin && src[it] >= 0;
      if (valid && !frmap_tally_finite_bits(__float_as_uint(xv[it]))) s_bad[it * 2 + lk] = 1;
      a[it] = valid ? frmap_head_fit_xp(xv[it], kb[it], keep_scale) : 0.0f;
      b[it] = (kin && c0 + it * 2 + lk < C) ? wv[it] : 0.0f;
    }
  }
};

// the operands of the update tile (c0, d0): A = g^T, B = x' of the batch rows (k = the batch row: consecutive lanes walk the tile
// row, which is contiguous in g and in x); `ones`: B is a column of ones in column 0, for db
struct HfUpdateOp {
  const float* x;
  const uint8_t* keep;
  const float* g;
  const int32_t* row_src;
  float keep_scale;
  int c0, d0, D, C, ones;
  __device__ __forceinline__ void load(int k0, int K, int li, int lk, float (&a)[16], float (&b)[16]) const {
    int src[16];
    float gv[16], xv[16];
    int kb[16];
    const size_t ci = (size_t)(c0 + li < C ? c0 + li : C - 1), di = (size_t)(d0 + li < D ? d0 + li : D - 1);
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int k = k0 + it * 2 + lk;
      src[it] = row_src[k < K ? k : K - 1];
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int k = k0 + it * 2 + lk;
      gv[it] = g[(size_t)(k < K ? k : K - 1) * (size_t)C + ci];
    }
    if (!ones) {                                                  // (uniform)
#pragma unroll
      for (int it = 0; it < 16; ++it) xv[it] = x[(size_t)(src[it] < 0 ? 0 : src[it]) * (size_t)D + di];
    }
    if (!ones && keep) {
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        const int k = k0 + it * 2 + lk;
        kb[it] = (int)keep[(size_t)(k < K ? k : K - 1) * (size_t)D + di];
      }
    } else {
#pragma unroll
      for (int it = 0; it < 16; ++it) kb[it] = -1;
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const bool valid = k0 + it * 2 + lk < K && src[it] >= 0;
      a[it] = (valid && c0 + li < C) ? gv[it] : 0.0f;
      if (ones) b[it] = (valid && li == 0) ? 1.0f : 0.0f;
      else b[it] = (valid && d0 + li < D) ? frmap_head_fit_xp(xv[it], kb[it], keep_scale) : 0.0f;
    }
  }
};

// The bodies of the three kernels are device functions over ALREADY-OFFSET pointers and by-value scalars: the single step's kernels
// hand them their arguments, the grouped step's kernels (blockIdx.z = the head) the slices of their head and its row of the hyper
// table.  The x and y of the grid mean the same in both, so head h of a group runs the instructions of the single step.
// HIDDEN: the first layer of the hidden-layer step - the same tile walk over w = w1 [C = Hd, D] with the ReLU epilogue; a label is
// in range below CL (the class count, where C is the hidden width), `lab` receives the label of a counted row or -1, and nothing is
// counted into any state.
// HF_PAIR_ROWS: the forward of the pair step (head_fit_pair.hip) - no label is read or checked, the identity epilogue, nothing counted;
// batch row i reads rows[i] below `split` and rows_hi[i - split] from there on.  (MODE was a bool: false / true still name the first two.)
// HF_MARGIN: the forward of the margin step (head_fit_margin.hip) - HF_LINEAR's labels, row_src and count of n, but no bias is read or added.
// HF_EMBED: the first layer of the embedding step (head_fit_embed.hip) - HF_HIDDEN's labels (in range below CL), lab and row_src and no
// count, with HF_MARGIN's epilogue: no bias is read or added and there is no ReLU.
constexpr int HF_LINEAR = 0, HF_HIDDEN = 1, HF_PAIR_ROWS = 2, HF_MARGIN = 3, HF_EMBED = 4;
template <int MODE>
__device__ __forceinline__ void hf_logits_body(const float* __restrict__ x, const int32_t* __restrict__ labels, const int32_t* __restrict__ rows,
                                               const uint8_t* __restrict__ keep, float keep_scale, const float* __restrict__ w,
                                               const float* __restrict__ b, uint64_t* state, float* __restrict__ z,
                                               int32_t* __restrict__ row_src, int32_t* __restrict__ lab, int N, int B, int D, int C, int CL,
                                               const int32_t* __restrict__ rows_hi = nullptr, int split = 0) {
  constexpr bool HIDDEN = MODE == HF_HIDDEN, LAB = MODE == HF_HIDDEN || MODE == HF_EMBED;
  __shared__ HfSmem sm;
  __shared__ int s_src[HF_T];        // the row of x behind tile row i; -1: outside the batch, the cache or the label range
  __shared__ int s_bad[HF_T];        // a non-finite feature was staged for tile row i
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * HF_T, b0 = blockIdx.y * HF_T;
  if (tid < HF_T) {
    int src = -1;
    const int i = b0 + tid;
    if (i < B) {
      if (MODE == HF_PAIR_ROWS) {
        const long long r = (long long)(i < split ? rows[i] : rows_hi[i - split]);
        if (r >= 0 && r < (long long)N) src = (int)r;
      } else {
        const long long r = rows ? (long long)rows[i] : (long long)i;
        if (r >= 0 && r < (long long)N) {
          const int y = labels[r];
          if (y >= 0 && y < (LAB ? CL : C)) src = (int)r;
        }
      }
    }
    s_src[tid] = src;
    s_bad[tid] = 0;
  }
  __syncthreads();
  const int vi = B - b0 < HF_T ? B - b0 : HF_T, vj = C - c0 < HF_T ? C - c0 : HF_T;
  float tot[4];
  const HfLogitsOp op = {x, keep, w, s_src, s_bad, keep_scale, b0, c0, B, D, C};
  hf_tile_chains<true, true>(sm, D, vi < HF_T || vj < HF_T, vi, vj, op, tot);
  __syncthreads();                   // every feature of the 32 rows has been staged by some wavefront: s_bad is final
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = (tid >> 5) + 8 * q, j = tid & 31;
    if (b0 + i < B && c0 + j < C) {
      const bool declined = s_src[i] < 0 || s_bad[i] != 0;
      if (HIDDEN) z[(size_t)(b0 + i) * (size_t)C + c0 + j] = declined ? 0.0f : frmap_head_fit_relu(tot[q] + b[c0 + j]);
      else if (MODE == HF_MARGIN || MODE == HF_EMBED) z[(size_t)(b0 + i) * (size_t)C + c0 + j] = declined ? 0.0f : tot[q];
      else z[(size_t)(b0 + i) * (size_t)C + c0 + j] = declined ? 0.0f : tot[q] + b[c0 + j];
    }
  }
  if (blockIdx.x == 0 && tid < 64) {
    const bool in = tid < HF_T && b0 + tid < B;
    const bool counted = in && s_src[tid] >= 0 && s_bad[tid] == 0;
    if (in) row_src[b0 + tid] = counted ? s_src[tid] : -1;
    if (MODE == HF_PAIR_ROWS) return;
    if (LAB) {
      if (in) lab[b0 + tid] = counted ? labels[s_src[tid]] : -1;
      return;
    }
    const unsigned long long m = __ballot(counted);
    if (tid == 0 && m) hf_add(state + FRMAP_HEAD_FIT_N, (uint64_t)__popcll(m));
  }
}

// `evaluate`: the figures only - t stays
__device__ __forceinline__ void hf_softmax_body(const int32_t* __restrict__ labels, const int32_t* __restrict__ row_src, uint64_t* state,
                                                const float* __restrict__ z, float* __restrict__ g, float* __restrict__ row_loss, int B, int C,
                                                float ls, bool evaluate) {
  __shared__ unsigned long long s_fig[HF_WAVES][2];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t n = state[FRMAP_HEAD_FIT_N];
  const FrmapHeadFitTarget tg = frmap_head_fit_target(ls, C);
  unsigned long long correct = 0ull, loss_q = 0ull;                // of this wavefront (wave-uniform)
  for (long long i = (long long)blockIdx.x * HF_WAVES + wave; i < (long long)B; i += (long long)gridDim.x * HF_WAVES) {
    const int src = row_src[i];
    const float* zr = z + (size_t)i * (size_t)C;
    float* gr = g + (size_t)i * (size_t)C;
    if (src < 0) {                                                 // (wave-uniform)
      for (int c = lane; c < C; c += 64) gr[c] = 0.0f;
      if (lane == 0) row_loss[i] = __builtin_nanf("");
      continue;
    }
    const int y = labels[src];
    const float zy = zr[y];
    float mx = -INFINITY;
    int mi = 0x7FFFFFFF;
    for (int c = lane; c < C; c += 64) {
      const float v = zr[c];
      if (v > mx || (v == mx && c < mi)) { mx = v; mi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mx, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
    }
    double sum = 0.0;                                               // float64 from here to the one rounding of g and the loss
    for (int c = lane; c < C; c += 64) sum += frmap_head_fit_exp(zr[c], mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const double lse = log(sum);
    double nl_sum = 0.0;
    if (ls > 0.0f) {
      for (int c = lane; c < C; c += 64) nl_sum += frmap_head_fit_nl(lse, zr[c], mx);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) nl_sum += __shfl_xor(nl_sum, o, 64);
    }
    const float loss = frmap_head_fit_loss(frmap_head_fit_nl(lse, zy, mx), nl_sum, ls, tg);
    for (int c = lane; c < C; c += 64) gr[c] = frmap_head_fit_g(frmap_head_fit_exp(zr[c], mx), sum, c == y ? tg.y_on : tg.y_off, n);
    if (lane == 0) row_loss[i] = loss;
    correct += mi == y ? 1 : 0;                                    // (a row of NaN logits has no arg-max: mi stays out of range)
    loss_q += frmap_tally_loss_q(loss);
  }
  if (lane == 0) {
    s_fig[wave][0] = correct;
    s_fig[wave][1] = loss_q;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long v = 0ull;
#pragma unroll
    for (int wv = 0; wv < HF_WAVES; ++wv) v += s_fig[wv][threadIdx.x];
    if (v) hf_add(state + (threadIdx.x == 0 ? FRMAP_HEAD_FIT_CORRECT : FRMAP_HEAD_FIT_LOSS_Q), v);
  }
  // nobody reads t or `rows` in this launch: the update kernel finds the step count already advanced
  if (blockIdx.x == 0 && threadIdx.x == 0 && n) {
    if (!evaluate) state[FRMAP_HEAD_FIT_T] += 1;
    state[FRMAP_HEAD_FIT_ROWS] += n;
  }
}

__device__ __forceinline__ void hf_update_body(const float* __restrict__ x, const uint8_t* __restrict__ keep, float keep_scale,
                                               float* __restrict__ w, float* __restrict__ b, void* state, const float* __restrict__ g,
                                               const int32_t* __restrict__ row_src, int B, int D, int C, const FrmapHeadFitHyper& h, int flags) {
  __shared__ HfSmem sm;
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0;
  const FrmapHeadFitState st = frmap_head_fit_state(state, D, C, amsgrad);
  if (st.head[FRMAP_HEAD_FIT_N] == 0) return;                      // every row declined: no weight, no moment changes (uniform)
  const FrmapHeadFitAdam a = frmap_head_fit_adam_scalars(st.head[FRMAP_HEAD_FIT_T], h, flags);
  const int tid = threadIdx.x;
  const int d0 = blockIdx.x * HF_T, c0 = blockIdx.y * HF_T;
  const int vi = C - c0 < HF_T ? C - c0 : HF_T;
  float tot[4];
  if (d0 >= D) {
    // The last column of workgroups owns db and the bias: the same chains against a column of ones (fmaf(g, 1, c) is c + g), on the
    // matrix cores where the class tile is full.  Column 0 of the tile is db; thread (i, 0) owns class c0 + i.
    const HfUpdateOp op = {x, keep, g, row_src, keep_scale, c0, 0, D, C, 1};
    hf_tile_chains<false, false>(sm, B, vi < HF_T, vi, 1, op, tot);
    if ((tid & 31) == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + (tid >> 5) + 8 * q;
        if (c < C) frmap_head_fit_adam(a, tot[q], b + c, st.m_b + c, st.v_b + c, amsgrad ? st.vmax_b + c : nullptr);
      }
    }
    return;
  }
  const int vj = D - d0 < HF_T ? D - d0 : HF_T;
  const HfUpdateOp op = {x, keep, g, row_src, keep_scale, c0, d0, D, C, 0};
  hf_tile_chains<false, false>(sm, B, vi < HF_T || vj < HF_T, vi, vj, op, tot);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = c0 + (tid >> 5) + 8 * q, d = d0 + (tid & 31);
    if (c < C && d < D) {
      const size_t at = (size_t)c * (size_t)D + d;
      frmap_head_fit_adam(a, tot[q], w + at, st.m_w + at, st.v_w + at, amsgrad ? st.vmax_w + at : nullptr);
    }
  }
}

// The update of the margin step (head_fit_rule.h, MARGIN): the tile (c0, d0) of w as in hf_update_body - the chains A = dot_i(g, x') -,
// then the one-column chain k = dot_i(h, 1) of the tile's 32 classes (every D-tile of a class row repeats it: B x 32 reads instead of a
// launch and a dependency across tiles; thread (i, 0) holds k of class c0 + i and hands it to its row through LDS), the combination
// frmap_head_fit_margin_dw with rw and Adam.  There is no bias and no bias column of workgroups.
__device__ __forceinline__ void hf_margin_update_body(const float* __restrict__ x, const uint8_t* __restrict__ keep, float keep_scale,
                                                      float* __restrict__ w, void* state, const float* __restrict__ g, const float* __restrict__ hm,
                                                      const float* __restrict__ rw, const int32_t* __restrict__ row_src, int B, int D, int C,
                                                      const FrmapHeadFitHyper& h, int flags) {
  __shared__ HfSmem sm;
  __shared__ float s_k[HF_T];
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0;
  const FrmapHeadFitState st = frmap_head_fit_state(state, D, C, amsgrad);
  if (st.head[FRMAP_HEAD_FIT_N] == 0) return;                      // every row declined: no weight, no moment changes (uniform)
  const FrmapHeadFitAdam a = frmap_head_fit_adam_scalars(st.head[FRMAP_HEAD_FIT_T], h, flags);
  const int tid = threadIdx.x;
  const int d0 = blockIdx.x * HF_T, c0 = blockIdx.y * HF_T;
  const int vi = C - c0 < HF_T ? C - c0 : HF_T, vj = D - d0 < HF_T ? D - d0 : HF_T;
  float tot[4], kk[4];
  const HfUpdateOp op = {x, keep, g, row_src, keep_scale, c0, d0, D, C, 0};
  hf_tile_chains<false, false>(sm, B, vi < HF_T || vj < HF_T, vi, vj, op, tot);
  const HfUpdateOp ones = {x, keep, hm, row_src, keep_scale, c0, 0, D, C, 1};
  hf_tile_chains<false, false>(sm, B, vi < HF_T, vi, 1, ones, kk);
  if ((tid & 31) == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s_k[(tid >> 5) + 8 * q] = kk[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = (tid >> 5) + 8 * q, c = c0 + i, d = d0 + (tid & 31);
    if (c < C && d < D) {
      const size_t at = (size_t)c * (size_t)D + d;
      const float dw = frmap_head_fit_margin_dw(tot[q], s_k[i], rw[c], w[at]);
      frmap_head_fit_adam(a, dw, w + at, st.m_w + at, st.v_w + at, amsgrad ? st.vmax_w + at : nullptr);
    }
  }
}
