// One training step of a contrastive pair head x -> normalize(x w^T + b) over pairs of cached rows (head_fit.PairHead.step,
// head_fit.fit_pair_head): the rule, the state and the workspace are head_fit_rule.h, PAIR; head_fit.pair_step_rule states the same in
// numpy and head_fit_twin.h on the host.  One small memset and four launches on the caller's stream, nothing copied to the host:
//   the memset of n (with `clear`: the figures), as the linear step does it;
//   head_fit_pair_forward_kernel  a = x' w^T + b over the 2P batch rows (row i < P reads left[i], row P + i right[i]): the logits tile
//                                 walk (hf_logits_body) with the identity epilogue and no labels.  It decides which ROWS are declined,
//                                 writes a and row_src, and counts nothing.
//   head_fit_pair_gate_kernel     one thread per pair: the pair is counted iff both rows are and differ is 0 or 1; an uncounted pair
//                                 gets -1 in row_src of both its rows; the counted pairs reach n as one integer atomic per wavefront.
//                                 n must be complete before any ga is formed (every ga carries 1 / n): that is this launch boundary.
//   head_fit_pair_kernel          one wavefront per pair, HF_WAVES pairs per workgroup, grid-stride over P.  Lanes stride over E and read
//                                 both rows coalesced; float64 wavefront sums of |a_l|^2 and |a_r|^2, then of |delta|^2, u . delta and
//                                 v . delta in one pass; then both rows of ga, pair_loss and dist, each rounded to fp32 once.  Up to
//                                 E = HF_PAIR_REG_E a lane keeps its elements of both rows in registers over the three passes; above it
//                                 the passes re-read them (they are this wavefront's own lines, in L2 by then).  The figures reach the
//                                 state as at most two integer atomics per workgroup; workgroup 0 advances t and adds n to `rows`
//                                 when n > 0.
//   head_fit_pair_update_kernel   the linear step's update body on (x, keep, g := ga, row_src) with B := 2P, C := E.
// No grid barrier, no flags between workgroups, no float atomics.  The wrappers around the shared bodies are this file's own kernels:
// head_fit.hip's and head_fit_hidden.hip's code objects do not change with this file.
#include "head_fit_launch.h"

constexpr int HF_PAIR_PER_LANE = 8;                       // elements of a row that a lane keeps in registers
constexpr int HF_PAIR_REG_E = 64 * HF_PAIR_PER_LANE;      // 512: 16 fp32 registers for the two rows; the reference's embedding is 256

__global__ __launch_bounds__(64 * HF_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void head_fit_pair_forward_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ left, const int32_t* __restrict__ right, const uint8_t* __restrict__ keep,
    float keep_scale, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ a, int32_t* __restrict__ row_src, int N, int P,
    int D, int E) {
  hf_logits_body<HF_PAIR_ROWS>(x, nullptr, left, keep, keep_scale, w, b, nullptr, a, row_src, nullptr, N, 2 * P, D, E, E, right, P);
}

__global__ __launch_bounds__(256) void head_fit_pair_gate_kernel(const int32_t* __restrict__ differ, int32_t* __restrict__ row_src, uint64_t* state,
                                                                 int P) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  bool counted = false;
  if (p < (long long)P) {
    const int dv = differ[p];
    counted = row_src[p] >= 0 && row_src[(size_t)P + (size_t)p] >= 0 && (dv == 0 || dv == 1);
    if (!counted) row_src[p] = row_src[(size_t)P + (size_t)p] = -1;
  }
  const unsigned long long m = __ballot(counted);
  if ((threadIdx.x & 63) == 0 && m) hf_add(state + FRMAP_HEAD_FIT_N, (uint64_t)__popcll(m));
}

__device__ __forceinline__ double hf_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The float64 half of one counted pair by one wavefront.  REG: E <= HF_PAIR_REG_E and element k of this lane is e = lane + 64 k, held
// in registers; else every pass reads the rows again.
template <bool REG>
__device__ __forceinline__ void hf_pair_one(const float* __restrict__ al, const float* __restrict__ ar, float* __restrict__ gl, float* __restrict__ gr,
                                            int E, int lane, int dv, uint64_t n, const FrmapHeadFitPairHyper& ph, FrmapHeadFitPair& pr) {
  float rl[HF_PAIR_PER_LANE], rr[HF_PAIR_PER_LANE];
  double nl2 = 0.0, nr2 = 0.0, dd = 0.0, ud = 0.0, vd = 0.0;
  if (REG) {
#pragma unroll
    for (int k = 0; k < HF_PAIR_PER_LANE; ++k) {
      const int e = lane + 64 * k;
      rl[k] = e < E ? al[e] : 0.0f;
      rr[k] = e < E ? ar[e] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < HF_PAIR_PER_LANE; ++k) {
      nl2 += (double)rl[k] * (double)rl[k];
      nr2 += (double)rr[k] * (double)rr[k];
    }
  } else {
    for (int e = lane; e < E; e += 64) {
      const double l = (double)al[e], r = (double)ar[e];
      nl2 += l * l;
      nr2 += r * r;
    }
  }
  frmap_head_fit_pair_norms(hf_wave_sum(nl2), hf_wave_sum(nr2), &pr);
  if (REG) {
#pragma unroll
    for (int k = 0; k < HF_PAIR_PER_LANE; ++k) {
      if (lane + 64 * k < E) {
        double u, v;
        const double delta = frmap_head_fit_pair_delta(rl[k], rr[k], pr.sl, pr.sr, &u, &v);
        dd += delta * delta;
        ud += u * delta;
        vd += v * delta;
      }
    }
  } else {
    for (int e = lane; e < E; e += 64) {
      double u, v;
      const double delta = frmap_head_fit_pair_delta(al[e], ar[e], pr.sl, pr.sr, &u, &v);
      dd += delta * delta;
      ud += u * delta;
      vd += v * delta;
    }
  }
  dd = hf_wave_sum(dd);
  ud = hf_wave_sum(ud);
  vd = hf_wave_sum(vd);
  frmap_head_fit_pair_scalars(dd, ud, vd, dv, n, ph, &pr);
  if (REG) {
#pragma unroll
    for (int k = 0; k < HF_PAIR_PER_LANE; ++k) {
      const int e = lane + 64 * k;
      if (e < E) frmap_head_fit_pair_ga(rl[k], rr[k], pr, gl + e, gr + e);
    }
  } else {
    for (int e = lane; e < E; e += 64) frmap_head_fit_pair_ga(al[e], ar[e], pr, gl + e, gr + e);
  }
}

__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_pair_kernel(const int32_t* __restrict__ differ, const int32_t* __restrict__ row_src,
                                                                      uint64_t* state, const float* __restrict__ a, float* __restrict__ ga,
                                                                      float* __restrict__ pair_loss, float* __restrict__ dist, int P, int E,
                                                                      FrmapHeadFitPairHyper ph) {
  __shared__ unsigned long long s_fig[HF_WAVES][2];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t n = state[FRMAP_HEAD_FIT_N];
  const size_t side = (size_t)P * (size_t)E;                        // from a pair's left row to its right row
  unsigned long long correct = 0ull, loss_q = 0ull;                 // of this wavefront (wave-uniform)
  for (long long p = (long long)blockIdx.x * HF_WAVES + wave; p < (long long)P; p += (long long)gridDim.x * HF_WAVES) {
    const size_t at = (size_t)p * (size_t)E;
    float* gl = ga + at;
    float* gr = ga + side + at;
    if (row_src[p] < 0) {                                           // (wave-uniform; the gate marked both rows of an uncounted pair)
      for (int e = lane; e < E; e += 64) gl[e] = gr[e] = 0.0f;
      if (lane == 0) pair_loss[p] = dist[p] = __builtin_nanf("");
      continue;
    }
    const int dv = differ[p];
    FrmapHeadFitPair pr;
    if (E <= HF_PAIR_REG_E) hf_pair_one<true>(a + at, a + side + at, gl, gr, E, lane, dv, n, ph, pr);      // (uniform)
    else hf_pair_one<false>(a + at, a + side + at, gl, gr, E, lane, dv, n, ph, pr);
    if (lane == 0) {
      pair_loss[p] = pr.loss;
      dist[p] = pr.dist;
    }
    correct += ((pr.dist < ph.accept) == (dv == 0)) ? 1 : 0;
    loss_q += frmap_tally_loss_q(pr.loss);
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
    state[FRMAP_HEAD_FIT_T] += 1;
    state[FRMAP_HEAD_FIT_ROWS] += n;
  }
}

__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_pair_update_kernel(const float* __restrict__ x, const uint8_t* __restrict__ keep,
                                                                             float keep_scale, float* __restrict__ w, float* __restrict__ b,
                                                                             void* state, const float* __restrict__ g,
                                                                             const int32_t* __restrict__ row_src, int B, int D, int C,
                                                                             FrmapHeadFitHyper h, int flags) {
  hf_update_body(x, keep, keep_scale, w, b, state, g, row_src, B, D, C, h, flags);
}

extern "C" size_t frmap_head_fit_pair_state_bytes(int D, int E, int amsgrad) {
  if (!frmap_head_fit_shape_ok(D, E)) return 0;
  return frmap_head_fit_state_size(D, E, amsgrad);
}

extern "C" size_t frmap_head_fit_pair_workspace_bytes(int P, int D, int E) {
  if (!frmap_head_fit_pair_shape_ok(P, D, E)) return 0;
  return frmap_head_fit_pair_workspace_size(P, E);
}

extern "C" int frmap_head_fit_pair_step(const float* x, const int32_t* left, const int32_t* right, const int32_t* differ, const uint8_t* keep,
                                        float keep_scale, float* w, float* b, void* state, void* workspace, int N, int P, int D, int E,
                                        float margin, float w_same, float w_diff, float accept, float lr, float beta1, float beta2, float eps,
                                        float weight_decay, int flags, void* stream) {
  const char* why = frmap_head_fit_pair_refusal(x, left, right, differ, w, b, state, workspace, N, P, D, E, flags);
  FRMAP_REQUIRE(!why, "head_fit_pair_step: %s (N = %d, P = %d, D = %d, E = %d, flags = %d)", why, N, P, D, E, flags);
  FRMAP_REQUIRE_ALIGNED(x, 4, "x");
  FRMAP_REQUIRE_ALIGNED(left, 4, "left");
  FRMAP_REQUIRE_ALIGNED(right, 4, "right");
  FRMAP_REQUIRE_ALIGNED(differ, 4, "differ");
  FRMAP_REQUIRE_ALIGNED(w, 4, "w");
  FRMAP_REQUIRE_ALIGNED(b, 4, "b");
  FRMAP_REQUIRE_ALIGNED(state, 8, "state");
  FRMAP_REQUIRE_ALIGNED(workspace, 4, "workspace");
  const hipStream_t st = (hipStream_t)stream;
  uint64_t* head = (uint64_t*)state;
  const FrmapHeadFitPairWork wk = frmap_head_fit_pair_work(workspace, P, E);
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, 0.0f};
  const FrmapHeadFitPairHyper ph = {margin, w_same, w_diff, accept};
  // n of the step in flight, and with `clear` the three epoch figures behind it (words 1 .. 4 of the header)
  if (hipMemsetAsync(head + FRMAP_HEAD_FIT_N, 0, (flags & FRMAP_HEAD_FIT_CLEAR) ? 32 : 8, st) != hipSuccess) {
    frmap_set_error("head_fit_pair_step: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
    return -2;
  }
  const int B = 2 * P;
  const unsigned tb = hf_tiles(B), te = hf_tiles(E), td = hf_tiles(D);
  const dim3 block(64 * HF_WAVES);
  hipLaunchKernelGGL(head_fit_pair_forward_kernel, dim3(te, tb), block, 0, st, x, left, right, keep, keep_scale, (const float*)w, (const float*)b,
                     wk.a, wk.row_src, N, P, D, E);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_pair_gate_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, differ, wk.row_src, head, P);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_pair_kernel, dim3(hf_softmax_blocks(P)), block, 0, st, differ, (const int32_t*)wk.row_src, head, (const float*)wk.a,
                     wk.ga, wk.pair_loss, wk.dist, P, E, ph);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_pair_update_kernel, dim3(td + 1, te), block, 0, st, x, keep, keep_scale, w, b, state, (const float*)wk.ga,
                     (const int32_t*)wk.row_src, B, D, E, h, flags);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" int frmap_head_fit_pair_step_host(const float* x_host, const int32_t* left_host, const int32_t* right_host, const int32_t* differ_host,
                                             const uint8_t* keep_host, float keep_scale, float* w_host, float* b_host, void* state_host,
                                             void* workspace_host, int N, int P, int D, int E, float margin, float w_same, float w_diff,
                                             float accept, float lr, float beta1, float beta2, float eps, float weight_decay, int flags,
                                             int given_g) {
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, 0.0f};
  const FrmapHeadFitPairHyper ph = {margin, w_same, w_diff, accept};
  const char* why = frmap_head_fit_pair_step_twin(x_host, left_host, right_host, differ_host, keep_host, keep_scale, w_host, b_host, state_host,
                                                  workspace_host, N, P, D, E, ph, h, flags, given_g);
  FRMAP_REQUIRE(!why, "head_fit_pair_step_host: %s (N = %d, P = %d, D = %d, E = %d, flags = %d)", why, N, P, D, E, flags);
  return 0;
}
