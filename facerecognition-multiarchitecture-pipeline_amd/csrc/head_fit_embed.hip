// One training step of the embedding layer of an ArcFace model - x -> x w1^T -> BatchNorm1d (training mode) -> dropout -> normalize ->
// margin -> cross-entropy, the frozen-trunk phase of the reference's two-phase ArcFace training - over cached pooled trunk features
// (head_fit.EmbedHead.step, head_fit.fit_embed_head): the rule, the state and the workspace are head_fit_rule.h, EMBED;
// head_fit.embed_step_rule states the same in numpy and head_fit_twin.h on the host.  One small memset and ten launches on the caller's
// stream, nothing copied to the host, nothing allocated:
//   head_fit_embed_forward_kernel      a = x w1^T: the logits tile walk (hf_logits_body) without a bias.  It decides layer 1's declined
//                                      rows as that body does, writes a, lab and row_src1 and counts nothing.
//   head_fit_embed_bn_forward_kernel   a workgroup owns 32 columns of a for all three passes over the batch (the sum, the squared
//                                      deviations, the normalisation), so no grid barrier is needed: 8 groups of 32 lanes, lanes across
//                                      the columns (a row of a is read as 128 contiguous bytes), a group strides over the rows.  The
//                                      float64 partial sums of the 8 groups meet in LDS and are added in ascending group order: the
//                                      same bits from run to run, no floating-point atomic.  It counts n1 on its way (every workgroup
//                                      the same; workgroup 0 stores it) and writes mean32, rstd, uvar, ah and y'.
//   the margin step's forward half     (frmap_head_fit_margin_forward_launch: its memset and its logits, norms and softmax kernels as
//                                      they are) on (y', lab) with the second header of the state as its header: n2 and the figures of
//                                      the step in flight land there, not in the epoch figures.
//   head_fit_embed_gate_kernel         one thread: the step is taken iff n1 >= 2 and n2 == n1.  It then advances t, adds the figures of
//                                      the step to the margin state and writes t and n into all three headers; else n = 0 in all
//                                      three, which is what every update kernel below returns on.  (head_fit_pair_gate_kernel is the
//                                      precedent of a gate launch.)
//   head_fit_embed_back_kernel         gy = gate (S - rx^2 k y'), S = (g rw) wc: a workgroup per 32 x 32 tile of gy over all k = C, in
//                                      head_fit_hidden_back_kernel's operand layout (A = g with k contiguous, scaled by rw[k] in the
//                                      loader - one fp32 product, the bits of a materialised gw -; B = wc with k the slow axis), then
//                                      the one-column chain k = dot_c(h, 1) of its 32 rows.  It reads wc, so it runs before the margin
//                                      update; the stream order gives that.
//   head_fit_embed_bn_backward_kernel  a workgroup owns 32 columns: the two chains over B (a group of 32 lanes walks a chain of 128
//                                      rows; the chains meet in LDS and are added in ascending order), then da, then Adam on gamma and
//                                      beta and the running statistics.  Every thread holds gamma of its column in a register before
//                                      the one thread of the column writes it.
//   head_fit_embed_update_kernel       the linear step's update body with g := da, C := E on (x, row_src1), no bias column of workgroups.
//   the margin step's update half      (frmap_head_fit_margin_update_launch) on (y', g, h, rw) and the third part of the state.
// No grid barrier, no flags between workgroups, no float atomics; integer atomics only where the shared bodies have them.
#include "head_fit_launch.h"

constexpr int HE_COLS = 32;                   // columns of a workgroup of the two BatchNorm kernels
constexpr int HE_GROUPS = 8;                  // groups of HE_COLS lanes: 256 threads

__global__ __launch_bounds__(64 * HF_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void head_fit_embed_forward_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ labels, const int32_t* __restrict__ rows, const float* __restrict__ w1,
    float* __restrict__ a, int32_t* __restrict__ row_src1, int32_t* __restrict__ lab, int N, int B, int D, int E, int C) {
  hf_logits_body<HF_EMBED>(x, labels, rows, nullptr, 1.0f, w1, nullptr, nullptr, a, row_src1, lab, N, B, D, E, C);
}

__global__ __launch_bounds__(HE_COLS * HE_GROUPS) void head_fit_embed_bn_forward_kernel(
    const float* __restrict__ a, const int32_t* __restrict__ row_src1, const uint8_t* __restrict__ keep, float keep_scale,
    const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ ah, float* __restrict__ yp,
    float* __restrict__ mean32, float* __restrict__ rstd, float* __restrict__ uvar, int32_t* __restrict__ n1_out, int B, int E, float bn_eps) {
  __shared__ double s_part[HE_GROUPS][HE_COLS];
  __shared__ int s_cnt[HE_GROUPS];
  const int tid = threadIdx.x, j = tid & (HE_COLS - 1), grp = tid >> 5;
  const int e = blockIdx.x * HE_COLS + j;
  const bool in = e < E;
  const size_t ec = (size_t)(in ? e : E - 1);                       // (a clamped, always valid column)
  // pass 1: the sum and the count of the counted rows
  double s = 0.0;
  int cnt = 0;
  for (int i = grp; i < B; i += HE_GROUPS) {
    if (row_src1[i] >= 0) {
      s += (double)a[(size_t)i * (size_t)E + ec];
      ++cnt;
    }
  }
  s_part[grp][j] = s;
  if (j == 0) s_cnt[grp] = cnt;
  __syncthreads();
  double tot = 0.0;
  int n1 = 0;
#pragma unroll
  for (int r = 0; r < HE_GROUPS; ++r) {
    tot += s_part[r][j];
    n1 += s_cnt[r];
  }
  __syncthreads();                                                  // s_part is free again
  const bool live = n1 >= 2;                                        // (uniform over the grid)
  const double mean = live ? tot / (double)n1 : 0.0;
  // pass 2: the squared deviations from the float64 mean
  double q = 0.0;
  if (live) {
    for (int i = grp; i < B; i += HE_GROUPS) {
      if (row_src1[i] >= 0) {
        const double d = (double)a[(size_t)i * (size_t)E + ec] - mean;
        q += d * d;
      }
    }
  }
  s_part[grp][j] = q;
  __syncthreads();
  double sq = 0.0;
#pragma unroll
  for (int r = 0; r < HE_GROUPS; ++r) sq += s_part[r][j];
  FrmapHeadFitBnStats st = {0.0f, 0.0f, 0.0f};
  if (live) st = frmap_head_fit_bn_stats(mean, sq, (uint64_t)n1, bn_eps);
  // pass 3: normalise, affine, dropout
  const float ga = gamma[ec], be = beta[ec];
  for (int i = grp; i < B; i += HE_GROUPS) {
    const size_t at = (size_t)i * (size_t)E + ec;
    float ahv = 0.0f, ypv = 0.0f;
    if (live && row_src1[i] >= 0) {
      ahv = frmap_head_fit_bn_ah(a[at], st.mean32, st.rstd);
      ypv = frmap_head_fit_bn_y(ahv, ga, be, keep ? (int)keep[at] : -1, keep_scale);
    }
    if (in) {
      ah[at] = ahv;
      yp[at] = ypv;
    }
  }
  if (grp == 0 && in) {
    mean32[e] = st.mean32;
    rstd[e] = st.rstd;
    uvar[e] = st.uvar;
  }
  if (blockIdx.x == 0 && tid == 0) {
    n1_out[0] = n1;
    n1_out[1] = 0;                                                  // (the padding word: the workspace is written whole)
  }
}

// One thread decides whether the step is taken (head_fit_rule.h, EMBED, "all or nothing") and writes the three headers.  head2 holds
// what the margin forward half counted for the step in flight: n2, its figures, a step count of its own that nobody reads.
__global__ void head_fit_embed_gate_kernel(uint64_t* head1, uint64_t* head2, uint64_t* head3, const int32_t* __restrict__ n1_in, int flags) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint64_t n1 = (uint64_t)*n1_in, n2 = head2[FRMAP_HEAD_FIT_N];
  const bool taken = n1 >= 2 && n2 == n1;
  if (flags & FRMAP_HEAD_FIT_CLEAR) head3[FRMAP_HEAD_FIT_ROWS] = head3[FRMAP_HEAD_FIT_CORRECT] = head3[FRMAP_HEAD_FIT_LOSS_Q] = 0;
  if (taken) {
    head3[FRMAP_HEAD_FIT_T] += 1;
    head3[FRMAP_HEAD_FIT_ROWS] += n1;
    head3[FRMAP_HEAD_FIT_CORRECT] += head2[FRMAP_HEAD_FIT_CORRECT];
    head3[FRMAP_HEAD_FIT_LOSS_Q] += head2[FRMAP_HEAD_FIT_LOSS_Q];
  }
  const uint64_t t = head3[FRMAP_HEAD_FIT_T], n = taken ? n1 : 0;
  head3[FRMAP_HEAD_FIT_N] = n;
  head1[FRMAP_HEAD_FIT_T] = head2[FRMAP_HEAD_FIT_T] = t;
  head1[FRMAP_HEAD_FIT_N] = head2[FRMAP_HEAD_FIT_N] = n;
  head2[FRMAP_HEAD_FIT_ROWS] = head2[FRMAP_HEAD_FIT_CORRECT] = head2[FRMAP_HEAD_FIT_LOSS_Q] = 0;
}

// the operands of the back tile (b0, e0) of S, k = the class: A = g rw of the batch rows (k is contiguous in g; one fp32 product in
// the loader), B = wc, whose k is the slow axis (consecutive lanes walk the embedding units of one class, contiguous in wc)
struct HfEmbedBackOp {
  const float* g;
  const float* rw;
  const float* wc;
  int b0, e0, B, E, C;
  __device__ __forceinline__ void load(int k0, int K, int li, int lk, float (&a)[16], float (&b)[16]) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float gv[16], wv[16];
    const int ka = k0 + li;
    const size_t kac = (size_t)(ka < K ? ka : K - 1), ei = (size_t)(e0 + li < E ? e0 + li : E - 1);
    const float rwv = rw[kac];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int bi = b0 + it * 2 + lk;
      gv[it] = g[(size_t)(bi < B ? bi : B - 1) * (size_t)C + kac];
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int k = k0 + it * 2 + lk;
      wv[it] = wc[(size_t)(k < K ? k : K - 1) * (size_t)E + ei];
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      a[it] = (ka < K && b0 + it * 2 + lk < B) ? gv[it] * rwv : 0.0f;
      b[it] = (k0 + it * 2 + lk < K && e0 + li < E) ? wv[it] : 0.0f;
    }
  }
};

// the operands of the one-column chain k[i] = dot_c(h[i][c], 1) of the tile's 32 batch rows: A = h (k contiguous), B = a column of
// ones in column 0
struct HfEmbedOnesOp {
  const float* h;
  int b0, B, C;
  __device__ __forceinline__ void load(int k0, int K, int li, int lk, float (&a)[16], float (&b)[16]) const {
    float hv[16];
    const int ka = k0 + li;
    const size_t kac = (size_t)(ka < K ? ka : K - 1);
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int bi = b0 + it * 2 + lk;
      hv[it] = h[(size_t)(bi < B ? bi : B - 1) * (size_t)C + kac];
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      a[it] = (ka < K && b0 + it * 2 + lk < B) ? hv[it] : 0.0f;
      b[it] = (k0 + it * 2 + lk < K && li == 0) ? 1.0f : 0.0f;
    }
  }
};

__global__ __launch_bounds__(64 * HF_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void head_fit_embed_back_kernel(
    const float* __restrict__ g, const float* __restrict__ hm, const float* __restrict__ rw, const float* __restrict__ rx,
    const float* __restrict__ wc, const float* __restrict__ yp, const uint8_t* __restrict__ keep, float keep_scale,
    const int32_t* __restrict__ row_src2, float* __restrict__ gy, int B, int E, int C) {
  __shared__ HfSmem sm;
  __shared__ float s_k[HF_T];
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * HF_T, b0 = blockIdx.y * HF_T;
  const int vi = B - b0 < HF_T ? B - b0 : HF_T, vj = E - e0 < HF_T ? E - e0 : HF_T;
  float tot[4], kk[4];
  const HfEmbedBackOp op = {g, rw, wc, b0, e0, B, E, C};
  hf_tile_chains<true, false>(sm, C, vi < HF_T || vj < HF_T, vi, vj, op, tot);
  const HfEmbedOnesOp ones = {hm, b0, B, C};
  hf_tile_chains<true, false>(sm, C, vi < HF_T, vi, 1, ones, kk);
  if ((tid & 31) == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s_k[(tid >> 5) + 8 * q] = kk[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int il = (tid >> 5) + 8 * q, i = b0 + il, e = e0 + (tid & 31);
    if (i < B && e < E) {
      const size_t at = (size_t)i * (size_t)E + e;
      gy[at] = row_src2[i] >= 0 ? frmap_head_fit_embed_gy(tot[q], s_k[il], rx[i], yp[at], keep ? (int)keep[at] : -1, keep_scale) : 0.0f;
    }
  }
}

__global__ __launch_bounds__(HE_COLS * HE_GROUPS) void head_fit_embed_bn_backward_kernel(
    const float* __restrict__ gy, const float* __restrict__ ah, const int32_t* __restrict__ row_src1, float* __restrict__ gamma,
    float* __restrict__ beta, const float* __restrict__ rstd, const float* __restrict__ mean32, const float* __restrict__ uvar,
    float* __restrict__ running_mean, float* __restrict__ running_var, const uint64_t* head1, void* state2, float* __restrict__ da,
    float* __restrict__ dbeta, float* __restrict__ dgamma, int B, int E, float bn_momentum, FrmapHeadFitHyper h, int flags) {
  __shared__ float s_b[HE_GROUPS][HE_COLS];
  __shared__ float s_g[HE_GROUPS][HE_COLS];
  const int tid = threadIdx.x, j = tid & (HE_COLS - 1), grp = tid >> 5;
  const int e = blockIdx.x * HE_COLS + j;
  const bool in = e < E;
  const size_t ec = (size_t)(in ? e : E - 1);
  const uint64_t n = head1[FRMAP_HEAD_FIT_N];                       // n1 of a step that is taken, else 0 (the gate kernel)
  const float ga = gamma[ec], rs = rstd[ec];                        // gamma BEFORE its update
  // dbeta = dot_i(gy, 1), dgamma = dot_i(gy, ah) in the rule's order: group r walks chain c0 + r, the chains are added ascending
  const int chains = (B + FRMAP_HEAD_FIT_CHAIN - 1) / FRMAP_HEAD_FIT_CHAIN;
  float tb = 0.0f, tg = 0.0f;
  for (int c0 = 0; c0 < chains; c0 += HE_GROUPS) {                  // (uniform: every barrier is reached by all)
    const int chain = c0 + grp;
    float cb = 0.0f, cg = 0.0f;
    if (chain < chains) {
      const int i1 = (chain + 1) * FRMAP_HEAD_FIT_CHAIN < B ? (chain + 1) * FRMAP_HEAD_FIT_CHAIN : B;
      for (int i = chain * FRMAP_HEAD_FIT_CHAIN; i < i1; ++i) {
        const bool ok = row_src1[i] >= 0;
        const size_t at = (size_t)i * (size_t)E + ec;
        const float gv = ok ? gy[at] : 0.0f, av = ok ? ah[at] : 0.0f;
        cb = fmaf(gv, 1.0f, cb);
        cg = fmaf(gv, av, cg);
      }
    }
    s_b[grp][j] = cb;
    s_g[grp][j] = cg;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < HE_GROUPS; ++r) {
      if (c0 + r < chains) {
        tb = tb + s_b[r][j];
        tg = tg + s_g[r][j];
      }
    }
    __syncthreads();
  }
  for (int i = grp; i < B; i += HE_GROUPS) {
    const size_t at = (size_t)i * (size_t)E + ec;
    const float v = (n && row_src1[i] >= 0) ? frmap_head_fit_bn_da(gy[at], ah[at], ga, rs, tb, tg, n) : 0.0f;
    if (in) da[at] = v;
  }
  __syncthreads();                                                  // every thread of the column has read gamma
  if (grp != 0 || !in) return;
  dbeta[e] = tb;
  dgamma[e] = tg;
  if (n == 0) return;                                               // the step is not taken: no parameter, moment or statistic moves
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0;
  const FrmapHeadFitState st = frmap_head_fit_state(state2, 1, E, amsgrad);
  const FrmapHeadFitAdam ad = frmap_head_fit_adam_scalars(head1[FRMAP_HEAD_FIT_T], h, flags);
  frmap_head_fit_adam(ad, tg, gamma + e, st.m_w + e, st.v_w + e, amsgrad ? st.vmax_w + e : nullptr);
  frmap_head_fit_adam(ad, tb, beta + e, st.m_b + e, st.v_b + e, amsgrad ? st.vmax_b + e : nullptr);
  running_mean[e] = frmap_head_fit_bn_running(running_mean[e], mean32[e], bn_momentum);
  running_var[e] = frmap_head_fit_bn_running(running_var[e], uvar[e], bn_momentum);
}

__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_embed_update_kernel(const float* __restrict__ x, float* __restrict__ w1, void* state,
                                                                              const float* __restrict__ da, const int32_t* __restrict__ row_src1,
                                                                              int B, int D, int E, FrmapHeadFitHyper h, int flags) {
  hf_update_body(x, nullptr, 1.0f, w1, nullptr, state, da, row_src1, B, D, E, h, flags);
}

extern "C" size_t frmap_head_fit_embed_state_bytes(int D, int E, int C, int amsgrad) {
  if (!frmap_head_fit_embed_shape_ok(D, E, C)) return 0;
  return frmap_head_fit_embed_state_size(D, E, C, amsgrad);
}

extern "C" size_t frmap_head_fit_embed_workspace_bytes(int B, int D, int E, int C) {
  if (!frmap_head_fit_embed_shape_ok(D, E, C) || B < 1 || B > FRMAP_HEAD_FIT_MAX_B) return 0;
  return frmap_head_fit_embed_workspace_size(B, E, C);
}

extern "C" int frmap_head_fit_embed_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale,
                                         float* w1, float* gamma, float* beta, float* running_mean, float* running_var, float* wc, void* state,
                                         void* workspace, int N, int B, int D, int E, int C, float bn_eps, float bn_momentum, float s, float m,
                                         float label_smoothing, float lr, float beta1, float beta2, float eps, float weight_decay, int flags,
                                         void* stream) {
  const char* why = frmap_head_fit_embed_refusal(x, labels, w1, gamma, beta, running_mean, running_var, wc, state, workspace, N, B, D, E, C, flags);
  FRMAP_REQUIRE(!why, "head_fit_embed_step: %s (N = %d, B = %d, D = %d, E = %d, C = %d, flags = %d)", why, N, B, D, E, C, flags);
  FRMAP_REQUIRE_ALIGNED(x, 4, "x");
  FRMAP_REQUIRE_ALIGNED(labels, 4, "labels");
  FRMAP_REQUIRE_ALIGNED(rows, 4, "rows");
  FRMAP_REQUIRE_ALIGNED(w1, 4, "w1");
  FRMAP_REQUIRE_ALIGNED(gamma, 4, "gamma");
  FRMAP_REQUIRE_ALIGNED(beta, 4, "beta");
  FRMAP_REQUIRE_ALIGNED(running_mean, 4, "running_mean");
  FRMAP_REQUIRE_ALIGNED(running_var, 4, "running_var");
  FRMAP_REQUIRE_ALIGNED(wc, 4, "wc");
  FRMAP_REQUIRE_ALIGNED(state, 8, "state");
  FRMAP_REQUIRE_ALIGNED(workspace, 4, "workspace");
  const hipStream_t st = (hipStream_t)stream;
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0;
  const FrmapHeadFitEmbedState es = frmap_head_fit_embed_state(state, D, E, C, amsgrad);
  const FrmapHeadFitEmbedWork wk = frmap_head_fit_embed_work(workspace, B, E);
  const FrmapHeadFitMarginWork mw = frmap_head_fit_margin_work(wk.margin, B, C);
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, label_smoothing};
  uint64_t *head1 = (uint64_t*)es.linear, *head2 = (uint64_t*)es.bn, *head3 = (uint64_t*)es.margin;
  const unsigned tb = hf_tiles(B), td = hf_tiles(D), te = hf_tiles(E);
  const dim3 block(64 * HF_WAVES), bn_block(HE_COLS * HE_GROUPS);
  hipLaunchKernelGGL(head_fit_embed_forward_kernel, dim3(te, tb), block, 0, st, x, labels, rows, (const float*)w1, wk.a, wk.row_src1, wk.lab, N, B,
                     D, E, C);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_embed_bn_forward_kernel, dim3(te), bn_block, 0, st, (const float*)wk.a, (const int32_t*)wk.row_src1, keep, keep_scale,
                     (const float*)gamma, (const float*)beta, wk.ah, wk.yp, wk.mean32, wk.rstd, wk.uvar, wk.n1, B, E, bn_eps);
  FRMAP_LAUNCH_CHECK();
  // the margin forward half on (y', lab): its header is the second one of the state, cleared (bit 4) for the step in flight
  int rc = frmap_head_fit_margin_forward_launch(wk.yp, wk.lab, nullptr, nullptr, 1.0f, wc, head2, wk.margin, B, B, E, C, s, m, label_smoothing,
                                                (flags & FRMAP_HEAD_FIT_EASY_MARGIN) | FRMAP_HEAD_FIT_CLEAR, st, "head_fit_embed_step");
  if (rc) return rc;
  hipLaunchKernelGGL(head_fit_embed_gate_kernel, dim3(1), dim3(64), 0, st, head1, head2, head3, (const int32_t*)wk.n1, flags);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_embed_back_kernel, dim3(te, tb), block, 0, st, (const float*)mw.g, (const float*)mw.h, (const float*)mw.rw,
                     (const float*)mw.rx, (const float*)wc, (const float*)wk.yp, keep, keep_scale, (const int32_t*)mw.row_src, wk.gy, B, E, C);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_embed_bn_backward_kernel, dim3(te), bn_block, 0, st, (const float*)wk.gy, (const float*)wk.ah,
                     (const int32_t*)wk.row_src1, gamma, beta, (const float*)wk.rstd, (const float*)wk.mean32, (const float*)wk.uvar, running_mean,
                     running_var, (const uint64_t*)head1, es.bn, wk.da, wk.dbeta, wk.dgamma, B, E, bn_momentum, h, flags);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_embed_update_kernel, dim3(td, te), block, 0, st, x, w1, es.linear, (const float*)wk.da,
                     (const int32_t*)wk.row_src1, B, D, E, h, flags);
  FRMAP_LAUNCH_CHECK();
  // wc changes only now, after gy was written from it
  return frmap_head_fit_margin_update_launch(wk.yp, nullptr, 1.0f, wc, es.margin, wk.margin, B, E, C, h, flags, st);
}

extern "C" int frmap_head_fit_embed_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep_host,
                                              float keep_scale, float* w1_host, float* gamma_host, float* beta_host, float* running_mean_host,
                                              float* running_var_host, float* wc_host, void* state_host, void* workspace_host, int N, int B,
                                              int D, int E, int C, float bn_eps, float bn_momentum, float s, float m, float label_smoothing,
                                              float lr, float beta1, float beta2, float eps, float weight_decay, int flags, int given) {
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, label_smoothing};
  const FrmapHeadFitMarginHyper mh = {s, m};
  const FrmapHeadFitBnHyper bh = {bn_eps, bn_momentum};
  const char* why = frmap_head_fit_embed_step_twin(x_host, labels_host, rows_host, keep_host, keep_scale, w1_host, gamma_host, beta_host,
                                                   running_mean_host, running_var_host, wc_host, state_host, workspace_host, N, B, D, E, C, bh, mh,
                                                   h, flags, given);
  FRMAP_REQUIRE(!why, "head_fit_embed_step_host: %s (N = %d, B = %d, D = %d, E = %d, C = %d, flags = %d, given = %d)", why, N, B, D, E, C, flags,
                given);
  return 0;
}
