// The host twin of head_fit.hip: one training step of head_fit_rule.h on host memory, in the rule's own order - every dot product
// is the chain of frmap_head_fit_dot.  With `given_g` the forward half is skipped: z, g and row_loss of the workspace are INPUTS
// (the device's own, whose exp / log are not the C library's), and the figures, the gradient GEMM and the update run on them, so
// that the twin's weights and moments can be compared with the kernel's word for word.  Plain C++: the library compiles it into
// frmap_head_fit_step_host, tools/head_fit_check.cpp into a stand-alone program.
#pragma once
#include "head_fit_rule.h"

// dot_k(a(k), b(k)), k = 0 .. K-1, in the rule's order
template <class FA, class FB>
inline float frmap_head_fit_dot(int K, FA a, FB b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float s = 0.0f;
  for (int k0 = 0; k0 < K; k0 += FRMAP_HEAD_FIT_CHAIN) {
    const int k1 = k0 + FRMAP_HEAD_FIT_CHAIN < K ? k0 + FRMAP_HEAD_FIT_CHAIN : K;
    float c = 0.0f;
    for (int k = k0; k < k1; ++k) c = fmaf(a(k), b(k), c);
    s = s + c;
  }
  return s;
}

// the row of x that batch row i reads, or -1 where the row is declined
inline int32_t frmap_head_fit_row_src(const float* x, const int32_t* labels, const int32_t* rows, int i, int N, int D, int C) {
  const int64_t r = rows ? (int64_t)rows[i] : (int64_t)i;
  if (r < 0 || r >= (int64_t)N) return -1;
  const int32_t y = labels[r];
  if (y < 0 || y >= C) return -1;
  for (int k = 0; k < D; ++k) {
    uint32_t u;
    __builtin_memcpy(&u, x + (size_t)r * (size_t)D + k, 4);
    if (!frmap_tally_finite_bits(u)) return -1;
  }
  return (int32_t)r;
}

// NULL, or why the call is refused (nothing written then)
inline const char* frmap_head_fit_step_twin(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale,
                                            float* w, float* b, void* state, void* workspace, int N, int B, int D, int C,
                                            const FrmapHeadFitHyper& h, int flags, int given_g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (N < 1) return "N is below 1";
  if (B < 1 || B > FRMAP_HEAD_FIT_MAX_B) return "B is outside [1, 2^20]";
  if (D < 1 || D > FRMAP_HEAD_FIT_MAX_D) return "D is outside [1, 65536]";
  if (C < 1 || C > FRMAP_HEAD_FIT_MAX_C) return "C is outside [1, 65536]";
  if (!x || !labels || !w || !b || !state || !workspace) return "null pointer";
  if (flags & ~7) return "unknown flag bits";
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0;
  const FrmapHeadFitState st = frmap_head_fit_state(state, D, C, amsgrad);
  const FrmapHeadFitWork wk = frmap_head_fit_work(workspace, B, C);
  if (flags & FRMAP_HEAD_FIT_CLEAR) st.head[FRMAP_HEAD_FIT_ROWS] = st.head[FRMAP_HEAD_FIT_CORRECT] = st.head[FRMAP_HEAD_FIT_LOSS_Q] = 0;
  uint64_t n = 0;
  for (int i = 0; i < B; ++i) {
    wk.row_src[i] = frmap_head_fit_row_src(x, labels, rows, i, N, D, C);
    n += wk.row_src[i] >= 0 ? 1 : 0;
  }
  st.head[FRMAP_HEAD_FIT_N] = n;
  auto xp = [&](int i, int k) -> float {                  // x' of batch row i (declined: +0)
    const int32_t r = wk.row_src[i];
    if (r < 0) return 0.0f;
    return frmap_head_fit_xp(x[(size_t)r * (size_t)D + k], keep ? (int)keep[(size_t)i * (size_t)D + k] : -1, keep_scale);
  };
  const FrmapHeadFitTarget tg = frmap_head_fit_target(h.label_smoothing, C);
  uint64_t correct = 0, loss_q = 0;
  for (int i = 0; i < B; ++i) {
    float* z = wk.z + (size_t)i * (size_t)C;
    float* g = wk.g + (size_t)i * (size_t)C;
    const int32_t r = wk.row_src[i];
    if (r < 0) {
      if (!given_g) {
        for (int c = 0; c < C; ++c) z[c] = g[c] = 0.0f;
        wk.row_loss[i] = __builtin_nanf("");
      }
      continue;
    }
    const int32_t y = labels[r];
    if (!given_g) {
      for (int c = 0; c < C; ++c) {
        const float* wc = w + (size_t)c * (size_t)D;
        const float s = frmap_head_fit_dot(D, [&](int k) { return xp(i, k); }, [&](int k) { return wc[k]; });
        z[c] = s + b[c];
      }
    }
    int pred = 0;
    for (int c = 1; c < C; ++c)
      if (z[c] > z[pred]) pred = c;
    if (!given_g) {
      const float m = z[pred];
      double s = 0.0;
      for (int c = 0; c < C; ++c) s = s + frmap_head_fit_exp(z[c], m);
      const double lse = log(s);
      double nl_sum = 0.0;
      if (h.label_smoothing > 0.0f)
        for (int c = 0; c < C; ++c) nl_sum = nl_sum + frmap_head_fit_nl(lse, z[c], m);
      wk.row_loss[i] = frmap_head_fit_loss(frmap_head_fit_nl(lse, z[y], m), nl_sum, h.label_smoothing, tg);
      for (int c = 0; c < C; ++c) g[c] = frmap_head_fit_g(frmap_head_fit_exp(z[c], m), s, c == y ? tg.y_on : tg.y_off, n);
    }
    correct += pred == y ? 1 : 0;
    loss_q += frmap_tally_loss_q(wk.row_loss[i]);
  }
  st.head[FRMAP_HEAD_FIT_ROWS] += n;
  st.head[FRMAP_HEAD_FIT_CORRECT] += correct;
  st.head[FRMAP_HEAD_FIT_LOSS_Q] += loss_q;
  if (n == 0) return nullptr;
  st.head[FRMAP_HEAD_FIT_T] += 1;
  const FrmapHeadFitAdam a = frmap_head_fit_adam_scalars(st.head[FRMAP_HEAD_FIT_T], h, flags);
  auto gg = [&](int i, int c) -> float { return wk.row_src[i] < 0 ? 0.0f : wk.g[(size_t)i * (size_t)C + c]; };
  for (int c = 0; c < C; ++c) {
    for (int d = 0; d < D; ++d) {
      const float dw = frmap_head_fit_dot(B, [&](int i) { return gg(i, c); }, [&](int i) { return xp(i, d); });
      const size_t at = (size_t)c * (size_t)D + d;
      frmap_head_fit_adam(a, dw, w + at, st.m_w + at, st.v_w + at, amsgrad ? st.vmax_w + at : nullptr);
    }
    const float db = frmap_head_fit_dot(B, [&](int i) { return gg(i, c); }, [](int) { return 1.0f; });
    frmap_head_fit_adam(a, db, b + c, st.m_b + c, st.v_b + c, amsgrad ? st.vmax_b + c : nullptr);
  }
  return nullptr;
}
