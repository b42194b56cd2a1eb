// One training step of an ArcFace margin head - the class centres w [C, D] of the reference's ArcMarginProduct under softmax
// cross-entropy - over cached embeddings (head_fit.MarginHead.step, head_fit.fit_margin_head): the rule, the state and the workspace are
// head_fit_rule.h, MARGIN; head_fit.margin_step_rule states the same in numpy and head_fit_twin.h on the host.  One small memset and
// four launches on the caller's stream, nothing copied to the host:
//   the memset of n (with `clear`: the figures), as the linear step does it;
//   head_fit_margin_logits_kernel   z = x' w^T: the logits tile walk (hf_logits_body) in its no-bias mode.  It decides which rows are
//                                   declined, writes z and row_src and counts n.
//   head_fit_margin_norms_kernel    one wavefront per row over the B batch rows (x' through rows and keep) and the C rows of w: lanes
//                                   stride over D (coalesced), a float64 wavefront sum of the squares, rx [B] and rw [C] rounded to fp32
//                                   once.  It decides for itself whether a batch row is declined (rx = +0) - every feature passes
//                                   through its loads -, so it does not depend on the launch before it.
//   head_fit_margin_softmax_kernel  one wavefront per row, HF_WAVES rows a workgroup, the grid capped and strided as hf_softmax_body's:
//                                   the target's acos / cos / sin once per row, then the arg-max, the float64 sum, lse, the optional
//                                   smoothing sum, and cosv, g, h and the row loss, each rounded to fp32 once.  The figures reach the
//                                   state as at most two integer atomics per workgroup; workgroup 0 advances t when n > 0.
//   head_fit_margin_update_kernel   hf_margin_update_body: a workgroup owns a 32 x 32 tile of w, runs the chains over g and the one-column
//                                   chain over h for its classes, forms dw with rw and applies Adam.
// No grid barrier, no flags between workgroups, no float atomics.  The wrappers around the shared bodies are this file's own kernels:
// the code objects of head_fit.hip, head_fit_hidden.hip and head_fit_pair.hip do not change with this file.
#include "head_fit_launch.h"

__global__ __launch_bounds__(64 * HF_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void head_fit_margin_logits_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ labels, const int32_t* __restrict__ rows, const uint8_t* __restrict__ keep,
    float keep_scale, const float* __restrict__ w, uint64_t* state, float* __restrict__ z, int32_t* __restrict__ row_src, int N, int B, int D,
    int C) {
  hf_logits_body<HF_MARGIN>(x, labels, rows, keep, keep_scale, w, nullptr, state, z, row_src, nullptr, N, B, D, C, C);
}

__device__ __forceinline__ double hf_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// rows 0 .. B-1 of the walk are the batch rows, rows B .. B+C-1 the rows of w
__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_margin_norms_kernel(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                                              const int32_t* __restrict__ rows, const uint8_t* __restrict__ keep,
                                                                              float keep_scale, const float* __restrict__ w, float* __restrict__ rx,
                                                                              float* __restrict__ rw, int N, int B, int D, int C) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const long long total = (long long)B + (long long)C;
  for (long long r = (long long)blockIdx.x * HF_WAVES + wave; r < total; r += (long long)gridDim.x * HF_WAVES) {
    double sq = 0.0;
    if (r >= (long long)B) {                                        // (wave-uniform) a row of w
      const int c = (int)(r - (long long)B);
      const float* wr = w + (size_t)c * (size_t)D;
      for (int k = lane; k < D; k += 64) {
        const double v = (double)wr[k];
        sq += v * v;
      }
      sq = hf_wave_sum(sq);
      if (lane == 0) rw[c] = frmap_head_fit_margin_rnorm(sq);
      continue;
    }
    const int i = (int)r;
    long long src = rows ? (long long)rows[i] : (long long)i;
    if (src < 0 || src >= (long long)N) src = -1;
    if (src >= 0) {
      const int y = labels[src];
      if (y < 0 || y >= C) src = -1;
    }
    bool bad = false;
    if (src >= 0) {                                                 // (wave-uniform)
      const float* xr = x + (size_t)src * (size_t)D;
      const uint8_t* kr = keep ? keep + (size_t)i * (size_t)D : nullptr;
      for (int k = lane; k < D; k += 64) {
        const float v = xr[k];
        bad = bad || !frmap_tally_finite_bits(__float_as_uint(v));
        const double xv = (double)frmap_head_fit_xp(v, kr ? (int)kr[k] : -1, keep_scale);
        sq += xv * xv;
      }
    }
    const bool declined = src < 0 || __ballot(bad) != 0ull;
    sq = hf_wave_sum(sq);
    if (lane == 0) rx[i] = declined ? 0.0f : frmap_head_fit_margin_rnorm(sq);
  }
}

__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_margin_softmax_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ row_src,
                                                                                uint64_t* state, const float* __restrict__ z,
                                                                                const float* __restrict__ rx, const float* __restrict__ rw,
                                                                                float* __restrict__ cosv, float* __restrict__ g, float* __restrict__ hm,
                                                                                float* __restrict__ row_loss, int B, int C, float s, float m, float ls,
                                                                                int easy) {
  __shared__ unsigned long long s_fig[HF_WAVES][2];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t n = state[FRMAP_HEAD_FIT_N];
  const FrmapHeadFitTarget tg = frmap_head_fit_target(ls, C);
  unsigned long long correct = 0ull, loss_q = 0ull;                // of this wavefront (wave-uniform)
  for (long long i = (long long)blockIdx.x * HF_WAVES + wave; i < (long long)B; i += (long long)gridDim.x * HF_WAVES) {
    const int src = row_src[i];
    const size_t at = (size_t)i * (size_t)C;
    const float* zr = z + at;
    float *cr = cosv + at, *gr = g + at, *hr = hm + at;
    if (src < 0) {                                                 // (wave-uniform)
      for (int c = lane; c < C; c += 64) cr[c] = gr[c] = hr[c] = 0.0f;
      if (lane == 0) row_loss[i] = __builtin_nanf("");
      continue;
    }
    const int y = labels[src];
    const float rxi = rx[i];
    // the target's margin: acos, cos and sin once per row (every lane forms the same values)
    int inside_y;
    double out_y, dfac_y;
    const double cs_y = frmap_head_fit_margin_clamp(frmap_head_fit_margin_cos(zr[y], rxi, rw[y]), &inside_y);
    frmap_head_fit_margin_target(cs_y, inside_y, m, easy, &out_y, &dfac_y);
    auto logit = [&](int c, double* cosine, int* inside) -> double {
      *cosine = frmap_head_fit_margin_cos(zr[c], rxi, rw[c]);
      return frmap_head_fit_margin_logit(frmap_head_fit_margin_clamp(*cosine, inside), c == y, out_y, s);
    };
    double cosine, mx = -INFINITY;
    int inside, mi = 0x7FFFFFFF;
    for (int c = lane; c < C; c += 64) {
      const double v = logit(c, &cosine, &inside);
      if (v > mx || (v == mx && c < mi)) { mx = v; mi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(mx, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
    }
    double sum = 0.0;
    for (int c = lane; c < C; c += 64) sum += exp(logit(c, &cosine, &inside) - mx);
    sum = hf_wave_sum(sum);
    const double lse = log(sum);
    double nl_sum = 0.0;
    if (ls > 0.0f) {
      for (int c = lane; c < C; c += 64) nl_sum += lse - (logit(c, &cosine, &inside) - mx);
      nl_sum = hf_wave_sum(nl_sum);
    }
    const float loss = frmap_head_fit_loss(lse - (logit(y, &cosine, &inside) - mx), nl_sum, ls, tg);
    for (int c = lane; c < C; c += 64) {
      const double l = logit(c, &cosine, &inside);
      int in2;
      cr[c] = (float)frmap_head_fit_margin_clamp(cosine, &in2);
      frmap_head_fit_margin_gh(exp(l - mx), sum, c == y ? tg.y_on : tg.y_off, s, n, c == y ? dfac_y : (inside ? 1.0 : 0.0), rxi, cosine, gr + c,
                               hr + c);
    }
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
    state[FRMAP_HEAD_FIT_T] += 1;
    state[FRMAP_HEAD_FIT_ROWS] += n;
  }
}

__global__ __launch_bounds__(64 * HF_WAVES) void head_fit_margin_update_kernel(const float* __restrict__ x, const uint8_t* __restrict__ keep,
                                                                               float keep_scale, float* __restrict__ w, void* state,
                                                                               const float* __restrict__ g, const float* __restrict__ hm,
                                                                               const float* __restrict__ rw, const int32_t* __restrict__ row_src, int B,
                                                                               int D, int C, FrmapHeadFitHyper h, int flags) {
  hf_margin_update_body(x, keep, keep_scale, w, state, g, hm, rw, row_src, B, D, C, h, flags);
}

// the two halves of the launcher (head_fit_launch.h): frmap_head_fit_margin_step runs them back to back, the embedding step around its own kernels
int frmap_head_fit_margin_forward_launch(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale,
                                         const float* w, uint64_t* head, void* workspace, int N, int B, int D, int C, float s, float m,
                                         float label_smoothing, int flags, hipStream_t st, const char* who) {
  const FrmapHeadFitMarginWork wk = frmap_head_fit_margin_work(workspace, B, C);
  // n of the step in flight, and with `clear` the three epoch figures behind it (words 1 .. 4 of the header)
  if (hipMemsetAsync(head + FRMAP_HEAD_FIT_N, 0, (flags & FRMAP_HEAD_FIT_CLEAR) ? 32 : 8, st) != hipSuccess) {
    frmap_set_error("%s: hipMemsetAsync failed: %s", who, hipGetErrorString(hipGetLastError()));
    return -2;
  }
  const unsigned tb = hf_tiles(B), tc = hf_tiles(C);
  const dim3 block(64 * HF_WAVES);
  hipLaunchKernelGGL(head_fit_margin_logits_kernel, dim3(tc, tb), block, 0, st, x, labels, rows, keep, keep_scale, w, head, wk.z, wk.row_src, N, B,
                     D, C);
  FRMAP_LAUNCH_CHECK();
  // (B + C <= 2^20 + 2^16: hf_softmax_blocks takes it)
  hipLaunchKernelGGL(head_fit_margin_norms_kernel, dim3(hf_softmax_blocks(B + C)), block, 0, st, x, labels, rows, keep, keep_scale, w, wk.rx, wk.rw,
                     N, B, D, C);
  FRMAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_fit_margin_softmax_kernel, dim3(hf_softmax_blocks(B)), block, 0, st, labels, (const int32_t*)wk.row_src, head,
                     (const float*)wk.z, (const float*)wk.rx, (const float*)wk.rw, wk.cosv, wk.g, wk.h, wk.row_loss, B, C, s, m, label_smoothing,
                     (flags & FRMAP_HEAD_FIT_EASY_MARGIN) ? 1 : 0);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

int frmap_head_fit_margin_update_launch(const float* x, const uint8_t* keep, float keep_scale, float* w, void* state, void* workspace, int B,
                                        int D, int C, const FrmapHeadFitHyper& h, int flags, hipStream_t st) {
  const FrmapHeadFitMarginWork wk = frmap_head_fit_margin_work(workspace, B, C);
  hipLaunchKernelGGL(head_fit_margin_update_kernel, dim3(hf_tiles(D), hf_tiles(C)), dim3(64 * HF_WAVES), 0, st, x, keep, keep_scale, w, state,
                     (const float*)wk.g, (const float*)wk.h, (const float*)wk.rw, (const int32_t*)wk.row_src, B, D, C, h, flags);
  FRMAP_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t frmap_head_fit_margin_state_bytes(int D, int C, int amsgrad) {
  if (!frmap_head_fit_shape_ok(D, C)) return 0;
  return frmap_head_fit_state_size(D, C, amsgrad);
}

extern "C" size_t frmap_head_fit_margin_workspace_bytes(int B, int D, int C) {
  if (!frmap_head_fit_shape_ok(D, C) || B < 1 || B > FRMAP_HEAD_FIT_MAX_B) return 0;
  return frmap_head_fit_margin_workspace_size(B, C);
}

extern "C" int frmap_head_fit_margin_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale,
                                          float* w, void* state, void* workspace, int N, int B, int D, int C, float s, float m,
                                          float label_smoothing, float lr, float beta1, float beta2, float eps, float weight_decay, int flags,
                                          void* stream) {
  const char* why = frmap_head_fit_margin_refusal(x, labels, w, state, workspace, N, B, D, C, flags);
  FRMAP_REQUIRE(!why, "head_fit_margin_step: %s (N = %d, B = %d, D = %d, C = %d, flags = %d)", why, N, B, D, C, flags);
  FRMAP_REQUIRE_ALIGNED(x, 4, "x");
  FRMAP_REQUIRE_ALIGNED(labels, 4, "labels");
  FRMAP_REQUIRE_ALIGNED(rows, 4, "rows");
  FRMAP_REQUIRE_ALIGNED(w, 4, "w");
  FRMAP_REQUIRE_ALIGNED(state, 8, "state");
  FRMAP_REQUIRE_ALIGNED(workspace, 4, "workspace");
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, label_smoothing};
  const int rc = frmap_head_fit_margin_forward_launch(x, labels, rows, keep, keep_scale, w, (uint64_t*)state, workspace, N, B, D, C, s, m,
                                                      label_smoothing, flags, (hipStream_t)stream, "head_fit_margin_step");
  if (rc) return rc;
  return frmap_head_fit_margin_update_launch(x, keep, keep_scale, w, state, workspace, B, D, C, h, flags, (hipStream_t)stream);
}

extern "C" int frmap_head_fit_margin_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep_host,
                                               float keep_scale, float* w_host, void* state_host, void* workspace_host, int N, int B, int D, int C,
                                               float s, float m, float label_smoothing, float lr, float beta1, float beta2, float eps,
                                               float weight_decay, int flags, int given_g) {
  const FrmapHeadFitHyper h = {lr, beta1, beta2, eps, weight_decay, label_smoothing};
  const FrmapHeadFitMarginHyper mh = {s, m};
  const char* why = frmap_head_fit_margin_step_twin(x_host, labels_host, rows_host, keep_host, keep_scale, w_host, state_host, workspace_host, N,
                                                    B, D, C, mh, h, flags, given_g);
  FRMAP_REQUIRE(!why, "head_fit_margin_step_host: %s (N = %d, B = %d, D = %d, C = %d, flags = %d)", why, N, B, D, C, flags);
  return 0;
}
