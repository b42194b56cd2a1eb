// The host twin of head_fit.hip: one training step of head_fit_rule.h on host memory, in the rule's own order - every dot product
// is the chain of frmap_head_fit_dot.  With `given_g` the forward half is skipped: z, g and row_loss of the workspace are INPUTS
// (the device's own, whose exp / log are not the C library's), and the figures, the gradient GEMM and the update run on them, so
// that the twin's weights and moments can be compared with the kernel's word for word.  Plain C++: the library compiles it into
// frmap_head_fit_step_host, tools/head_fit_check.cpp into a stand-alone program.
// frmap_head_fit_group_step_twin is the grouped step (head_fit_rule.h, GROUPS): this twin on the slices of every head, with the
// stride, the hyper table and flag 8 of the device's (frmap_head_fit_group_step_host, tools/head_fit_group_check.cpp).
// frmap_head_fit_hidden_step_twin is the hidden-layer step (head_fit_rule.h, HIDDEN LAYER): layer 1 by frmap_head_fit_dot, all of
// layer 2 by this twin on (h, lab, keep2) (frmap_head_fit_hidden_step_host, tools/head_fit_hidden_check.cpp).
// frmap_head_fit_pair_step_twin is the pair step (head_fit_rule.h, PAIR): the projection and the update by frmap_head_fit_dot, the
// float64 loss and gradient of every pair in between (frmap_head_fit_pair_step_host, tools/head_fit_pair_check.cpp).
// frmap_head_fit_margin_step_twin is the margin step (head_fit_rule.h, MARGIN; frmap_head_fit_margin_step_host, tools/head_fit_margin_check.cpp).
// frmap_head_fit_embed_step_twin is the embedding step (head_fit_rule.h, EMBED): layer 1 and every chain by frmap_head_fit_dot, the batch
// statistics with serial float64 sums, the margin twin on (y', lab) for the margin stage (frmap_head_fit_embed_step_host,
// tools/head_fit_embed_check.cpp).
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

// What a head-fitting call is refused for, before anything is read or written: NULL, or the text (it names the argument).  This is
// the ONE list of the checks every step shares - the launchers and the twins of the single, the grouped and the hidden-layer step all
// begin with it, so that what the device refuses is what the twin refuses -, in this order: N, B, D, C, the flag bits outside
// `allowed` (7; 15 where FRMAP_HEAD_FIT_EVAL is a flag of the call), the `n_required` pointers that may not be NULL (`null_text`
// lists them).
inline const char* frmap_head_fit_refusal(int N, int B, int D, int C, int flags, int allowed, const void* const* required, int n_required,
                                          const char* null_text) {
  if (N < 1) return "N is below 1";
  if (B < 1 || B > FRMAP_HEAD_FIT_MAX_B) return "B is outside [1, 2^20]";
  if (D < 1 || D > FRMAP_HEAD_FIT_MAX_D) return "D is outside [1, 65536]";
  if (C < 1 || C > FRMAP_HEAD_FIT_MAX_C) return "C is outside [1, 65536]";
  if (flags & ~allowed)
    return (allowed & FRMAP_HEAD_FIT_EVAL)          ? "flags has unknown bits (1 decoupled, 2 amsgrad, 4 clear, 8 evaluate only)"
           : (allowed & FRMAP_HEAD_FIT_EASY_MARGIN) ? "flags has unknown bits (1 decoupled, 2 amsgrad, 4 clear, 16 easy margin)"
                                                    : "flags has unknown bits (1 decoupled, 2 amsgrad, 4 clear)";
  for (int k = 0; k < n_required; ++k)
    if (!required[k]) return null_text;
  return nullptr;
}

// the same for the operands of a linear head, single or grouped
inline const char* frmap_head_fit_linear_refusal(const void* x, const void* labels, const void* w, const void* b, const void* state,
                                                 const void* workspace, int N, int B, int D, int C, int flags, int allowed) {
  const void* const required[] = {x, labels, w, b, state, workspace};
  return frmap_head_fit_refusal(N, B, D, C, flags, allowed, required, 6, "null pointer (x, labels, w, b, state and workspace are required)");
}

// NULL, or why the call is refused (nothing written then).  `flags` may carry FRMAP_HEAD_FIT_EVAL (the grouped step's bit 8): the
// forward half and the figures only.
inline const char* frmap_head_fit_step_twin_any(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale,
                                                float* w, float* b, void* state, void* workspace, int N, int B, int D, int C,
                                                const FrmapHeadFitHyper& h, int flags, int given_g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (const char* why = frmap_head_fit_linear_refusal(x, labels, w, b, state, workspace, N, B, D, C, flags, 15)) return why;
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
  if (n == 0 || (flags & FRMAP_HEAD_FIT_EVAL)) return nullptr;
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

// the single step: bits 1, 2 and 4 of `flags`
inline const char* frmap_head_fit_step_twin(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale,
                                            float* w, float* b, void* state, void* workspace, int N, int B, int D, int C,
                                            const FrmapHeadFitHyper& h, int flags, int given_g) {
  if (const char* why = frmap_head_fit_linear_refusal(x, labels, w, b, state, workspace, N, B, D, C, flags, 7)) return why;
  return frmap_head_fit_step_twin_any(x, labels, rows, keep, keep_scale, w, b, state, workspace, N, B, D, C, h, flags, given_g);
}

// what a grouped call is refused for: the shared list, then what only a group has
inline const char* frmap_head_fit_group_refusal(const void* x, const void* labels, const void* rows, const void* keep, const void* hyper,
                                                const void* w, const void* b, const void* state, const void* workspace, int N, int H, int B,
                                                int D, int C, int flags) {
  if (const char* why = frmap_head_fit_linear_refusal(x, labels, w, b, state, workspace, N, B, D, C, flags, 15)) return why;
  if (H < 1 || H > FRMAP_HEAD_FIT_MAX_H) return "H is outside [1, 4096]";
  if (!rows) return "rows is NULL (a grouped step takes the rows of every head)";
  if (!hyper) return "hyper is NULL";
  if (keep && (flags & FRMAP_HEAD_FIT_EVAL)) return "keep is given with flag 8 (evaluate only takes no dropout mask)";
  if (!frmap_head_fit_group_fits(H, B, D, C, (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0)) return "H, B, D, C give a byte count past 64 bits";
  return nullptr;
}

// the hyper-parameters of head h: row h of the table, the values the single step takes by value
inline FrmapHeadFitHyper frmap_head_fit_group_hyper(const float* hyper, int h, float* keep_scale) {
  const float* r = hyper + (size_t)h * FRMAP_HEAD_FIT_HYPER_COLS;
  const FrmapHeadFitHyper hy = {r[0], r[1], r[2], r[3], r[4], r[5]};
  *keep_scale = r[FRMAP_HEAD_FIT_HYPER_KEEP_SCALE];
  return hy;
}

// The grouped step: the single twin on the slices of every head, in ascending h.  `given_g` per head as in the single twin.
inline const char* frmap_head_fit_group_step_twin(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep,
                                                  const float* hyper, float* w, float* b, void* state, void* workspace, int N, int H, int B,
                                                  int D, int C, int flags, int given_g) {
  const char* why = frmap_head_fit_group_refusal(x, labels, rows, keep, hyper, w, b, state, workspace, N, H, B, D, C, flags);
  if (why) return why;
  const size_t stride = frmap_head_fit_group_stride(D, C, (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0), work = frmap_head_fit_workspace_size(B, C);
  const size_t cd = (size_t)C * (size_t)D, bd = (size_t)B * (size_t)D;
  for (int h = 0; h < H; ++h) {
    float keep_scale;
    const FrmapHeadFitHyper hy = frmap_head_fit_group_hyper(hyper, h, &keep_scale);
    why = frmap_head_fit_step_twin_any(x, labels, rows + (size_t)h * (size_t)B, keep ? keep + (size_t)h * bd : nullptr, keep_scale,
                                       w + (size_t)h * cd, b + (size_t)h * (size_t)C, (char*)state + (size_t)h * stride,
                                       (char*)workspace + (size_t)h * work, N, B, D, C, hy, flags, given_g);
    if (why) return why;
  }
  return nullptr;
}

// what a hidden-layer call is refused for: the shared list, then what only it has
inline const char* frmap_head_fit_hidden_refusal(const void* x, const void* labels, const void* w1, const void* b1, const void* w2, const void* b2,
                                                 const void* state, const void* workspace, int N, int B, int D, int Hd, int C, int flags) {
  const void* const required[] = {x, labels, w1, b1, w2, b2, state, workspace};
  if (const char* why = frmap_head_fit_refusal(N, B, D, C, flags, 7, required, 8,
                                               "null pointer (x, labels, w1, b1, w2, b2, state and workspace are required)"))
    return why;
  if (Hd < 1 || Hd > FRMAP_HEAD_FIT_MAX_D) return "Hd is outside [1, 65536]";
  return nullptr;
}

// The hidden-layer step (head_fit_rule.h, HIDDEN LAYER): layer 1 forward by frmap_head_fit_dot, the single twin on (h, lab, keep2)
// for all of layer 2, then da against the w2 from BEFORE that update and layer 1's update.  `given_g` as in the single twin: z, g
// and row_loss of the layer-2 workspace are inputs.
inline const char* frmap_head_fit_hidden_step_twin(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep1,
                                                   float keep1_scale, const uint8_t* keep2, float keep2_scale, float* w1, float* b1, float* w2,
                                                   float* b2, void* state, void* workspace, int N, int B, int D, int Hd, int C,
                                                   const FrmapHeadFitHyper& h, int flags, int given_g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const char* why = frmap_head_fit_hidden_refusal(x, labels, w1, b1, w2, b2, state, workspace, N, B, D, Hd, C, flags);
  if (why) return why;
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0;
  void* state2 = (char*)state + frmap_head_fit_state_size(D, Hd, amsgrad);
  const FrmapHeadFitState st1 = frmap_head_fit_state(state, D, Hd, amsgrad);
  const FrmapHeadFitState st2 = frmap_head_fit_state(state2, Hd, C, amsgrad);
  const FrmapHeadFitHiddenWork wk = frmap_head_fit_hidden_work(workspace, B, Hd);
  const FrmapHeadFitWork wk2 = frmap_head_fit_work(wk.layer2, B, C);
  auto xp = [&](int i, int k) -> float {                  // x' of batch row i (declined by layer 1: +0)
    const int32_t r = wk.row_src1[i];
    if (r < 0) return 0.0f;
    return frmap_head_fit_xp(x[(size_t)r * (size_t)D + k], keep1 ? (int)keep1[(size_t)i * (size_t)D + k] : -1, keep1_scale);
  };
  for (int i = 0; i < B; ++i) {
    const int32_t r = wk.row_src1[i] = frmap_head_fit_row_src(x, labels, rows, i, N, D, C);
    wk.lab[i] = r < 0 ? -1 : labels[r];
    float* hr = wk.h + (size_t)i * (size_t)Hd;
    for (int j = 0; j < Hd; ++j) {
      if (r < 0) {
        hr[j] = 0.0f;
        continue;
      }
      const float* wj = w1 + (size_t)j * (size_t)D;
      const float s = frmap_head_fit_dot(D, [&](int k) { return xp(i, k); }, [&](int k) { return wj[k]; });
      hr[j] = frmap_head_fit_relu(s + b1[j]);
    }
  }
  // s needs w2 as it is before layer 2's update
  const size_t n_w2 = (size_t)C * (size_t)Hd;
  float* w2_old = new float[n_w2];
  for (size_t k = 0; k < n_w2; ++k) w2_old[k] = w2[k];
  why = frmap_head_fit_step_twin(wk.h, wk.lab, nullptr, keep2, keep2_scale, w2, b2, state2, wk.layer2, B, B, Hd, C, h, flags, given_g);
  if (why) {
    delete[] w2_old;
    return why;
  }
  for (int i = 0; i < B; ++i) {
    const bool counted = wk2.row_src[i] >= 0;
    const float* gr = wk2.g + (size_t)i * (size_t)C;
    for (int j = 0; j < Hd; ++j) {
      const size_t at = (size_t)i * (size_t)Hd + j;
      const float s = frmap_head_fit_dot(C, [&](int c) { return gr[c]; }, [&](int c) { return w2_old[(size_t)c * (size_t)Hd + j]; });
      wk.da[at] = frmap_head_fit_da(s, wk.h[at], keep2 ? (int)keep2[at] : -1, keep2_scale, counted);
    }
  }
  delete[] w2_old;
  const uint64_t n = st2.head[FRMAP_HEAD_FIT_N];
  st1.head[FRMAP_HEAD_FIT_T] = st2.head[FRMAP_HEAD_FIT_T];
  st1.head[FRMAP_HEAD_FIT_N] = n;
  if (n == 0) return nullptr;
  const FrmapHeadFitAdam a = frmap_head_fit_adam_scalars(st1.head[FRMAP_HEAD_FIT_T], h, flags);
  auto dd = [&](int i, int j) -> float { return wk.row_src1[i] < 0 ? 0.0f : wk.da[(size_t)i * (size_t)Hd + j]; };
  for (int j = 0; j < Hd; ++j) {
    for (int d = 0; d < D; ++d) {
      const float dw = frmap_head_fit_dot(B, [&](int i) { return dd(i, j); }, [&](int i) { return xp(i, d); });
      const size_t at = (size_t)j * (size_t)D + d;
      frmap_head_fit_adam(a, dw, w1 + at, st1.m_w + at, st1.v_w + at, amsgrad ? st1.vmax_w + at : nullptr);
    }
    const float db = frmap_head_fit_dot(B, [&](int i) { return dd(i, j); }, [](int) { return 1.0f; });
    frmap_head_fit_adam(a, db, b1 + j, st1.m_b + j, st1.v_b + j, amsgrad ? st1.vmax_b + j : nullptr);
  }
  return nullptr;
}

// what a pair call is refused for: the shared list in its order - N, P (where the others have B: 2P batch rows), D, E (where they have C),
// the flag bits, the required pointers
inline const char* frmap_head_fit_pair_refusal(const void* x, const void* left, const void* right, const void* differ, const void* w, const void* b,
                                               const void* state, const void* workspace, int N, int P, int D, int E, int flags) {
  const bool p_ok = P >= 1 && P <= FRMAP_HEAD_FIT_MAX_P, e_ok = E >= 1 && E <= FRMAP_HEAD_FIT_MAX_C;
  if (N >= 1) {
    if (!p_ok) return "P is outside [1, 2^19]";
    if (D >= 1 && D <= FRMAP_HEAD_FIT_MAX_D && !e_ok) return "E is outside [1, 65536]";
  }
  const void* const required[] = {x, left, right, differ, w, b, state, workspace};
  return frmap_head_fit_refusal(N, p_ok ? 2 * P : 1, D, e_ok ? E : 1, flags, 7, required, 8,
                                "null pointer (x, left, right, differ, w, b, state and workspace are required)");
}

// the row of x that a batch row of the pair step reads through index r, or -1 where it is declined (no label is read)
inline int32_t frmap_head_fit_pair_row_src(const float* x, int32_t r, int N, int D) {
  if (r < 0 || r >= N) return -1;
  for (int k = 0; k < D; ++k) {
    uint32_t u;
    __builtin_memcpy(&u, x + (size_t)r * (size_t)D + k, 4);
    if (!frmap_tally_finite_bits(u)) return -1;
  }
  return r;
}

// The pair step (head_fit_rule.h, PAIR): the projection by frmap_head_fit_dot, the counting, the float64 loss and gradient of every
// counted pair with serial sums, the figures, then the linear step's gradient GEMM and update on (ga, row_src) over the 2P rows.
// `given_g`: a, ga, pair_loss and dist of the workspace are INPUTS (the device's own); row_src, n, the figures and the update are
// computed from them.
inline const char* frmap_head_fit_pair_step_twin(const float* x, const int32_t* left, const int32_t* right, const int32_t* differ,
                                                 const uint8_t* keep, float keep_scale, float* w, float* b, void* state, void* workspace, int N,
                                                 int P, int D, int E, const FrmapHeadFitPairHyper& ph, const FrmapHeadFitHyper& h, int flags,
                                                 int given_g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (const char* why = frmap_head_fit_pair_refusal(x, left, right, differ, w, b, state, workspace, N, P, D, E, flags)) return why;
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0, B = 2 * P;
  const FrmapHeadFitState st = frmap_head_fit_state(state, D, E, amsgrad);
  const FrmapHeadFitPairWork wk = frmap_head_fit_pair_work(workspace, P, E);
  if (flags & FRMAP_HEAD_FIT_CLEAR) st.head[FRMAP_HEAD_FIT_ROWS] = st.head[FRMAP_HEAD_FIT_CORRECT] = st.head[FRMAP_HEAD_FIT_LOSS_Q] = 0;
  for (int i = 0; i < B; ++i) wk.row_src[i] = frmap_head_fit_pair_row_src(x, i < P ? left[i] : right[i - P], N, D);
  auto xp = [&](int i, int k) -> float {                  // x' of batch row i (declined: +0)
    const int32_t r = wk.row_src[i];
    if (r < 0) return 0.0f;
    return frmap_head_fit_xp(x[(size_t)r * (size_t)D + k], keep ? (int)keep[(size_t)i * (size_t)D + k] : -1, keep_scale);
  };
  if (!given_g) {
    for (int i = 0; i < B; ++i) {                         // (before the gate: a row of an uncounted pair keeps its projection)
      float* ar = wk.a + (size_t)i * (size_t)E;
      for (int e = 0; e < E; ++e) {
        if (wk.row_src[i] < 0) {
          ar[e] = 0.0f;
          continue;
        }
        const float* we = w + (size_t)e * (size_t)D;
        const float s = frmap_head_fit_dot(D, [&](int k) { return xp(i, k); }, [&](int k) { return we[k]; });
        ar[e] = s + b[e];
      }
    }
  }
  uint64_t n = 0;
  for (int p = 0; p < P; ++p) {
    const bool counted = wk.row_src[p] >= 0 && wk.row_src[P + p] >= 0 && (differ[p] == 0 || differ[p] == 1);
    if (!counted) wk.row_src[p] = wk.row_src[P + p] = -1;
    n += counted ? 1 : 0;
  }
  st.head[FRMAP_HEAD_FIT_N] = n;
  uint64_t correct = 0, loss_q = 0;
  for (int p = 0; p < P; ++p) {
    const float* al = wk.a + (size_t)p * (size_t)E;
    const float* ar = wk.a + (size_t)(P + p) * (size_t)E;
    float* gl = wk.ga + (size_t)p * (size_t)E;
    float* gr = wk.ga + (size_t)(P + p) * (size_t)E;
    if (wk.row_src[p] < 0) {
      if (!given_g) {
        for (int e = 0; e < E; ++e) gl[e] = gr[e] = 0.0f;
        wk.pair_loss[p] = wk.dist[p] = __builtin_nanf("");
      }
      continue;
    }
    if (!given_g) {
      FrmapHeadFitPair pr;
      double nl2 = 0.0, nr2 = 0.0, dd = 0.0, ud = 0.0, vd = 0.0;
      for (int e = 0; e < E; ++e) {
        nl2 = nl2 + (double)al[e] * (double)al[e];
        nr2 = nr2 + (double)ar[e] * (double)ar[e];
      }
      frmap_head_fit_pair_norms(nl2, nr2, &pr);
      for (int e = 0; e < E; ++e) {
        double u, v;
        const double delta = frmap_head_fit_pair_delta(al[e], ar[e], pr.sl, pr.sr, &u, &v);
        dd = dd + delta * delta;
        ud = ud + u * delta;
        vd = vd + v * delta;
      }
      frmap_head_fit_pair_scalars(dd, ud, vd, differ[p], n, ph, &pr);
      for (int e = 0; e < E; ++e) frmap_head_fit_pair_ga(al[e], ar[e], pr, gl + e, gr + e);
      wk.pair_loss[p] = pr.loss;
      wk.dist[p] = pr.dist;
    }
    correct += ((wk.dist[p] < ph.accept) == (differ[p] == 0)) ? 1 : 0;
    loss_q += frmap_tally_loss_q(wk.pair_loss[p]);
  }
  st.head[FRMAP_HEAD_FIT_ROWS] += n;
  st.head[FRMAP_HEAD_FIT_CORRECT] += correct;
  st.head[FRMAP_HEAD_FIT_LOSS_Q] += loss_q;
  if (n == 0) return nullptr;
  st.head[FRMAP_HEAD_FIT_T] += 1;
  const FrmapHeadFitAdam a = frmap_head_fit_adam_scalars(st.head[FRMAP_HEAD_FIT_T], h, flags);
  auto gg = [&](int i, int e) -> float { return wk.row_src[i] < 0 ? 0.0f : wk.ga[(size_t)i * (size_t)E + e]; };
  for (int e = 0; e < E; ++e) {
    for (int d = 0; d < D; ++d) {
      const float dw = frmap_head_fit_dot(B, [&](int i) { return gg(i, e); }, [&](int i) { return xp(i, d); });
      const size_t at = (size_t)e * (size_t)D + d;
      frmap_head_fit_adam(a, dw, w + at, st.m_w + at, st.v_w + at, amsgrad ? st.vmax_w + at : nullptr);
    }
    const float db = frmap_head_fit_dot(B, [&](int i) { return gg(i, e); }, [](int) { return 1.0f; });
    frmap_head_fit_adam(a, db, b + e, st.m_b + e, st.v_b + e, amsgrad ? st.vmax_b + e : nullptr);
  }
  return nullptr;
}

// what a margin call is refused for: the shared list (there is no bias; bit 16 of the flags is the easy margin)
struct FrmapHeadFitMarginHyper {
  float s, m;
};
inline const char* frmap_head_fit_margin_refusal(const void* x, const void* labels, const void* w, const void* state, const void* workspace, int N,
                                                 int B, int D, int C, int flags) {
  const void* const required[] = {x, labels, w, state, workspace};
  return frmap_head_fit_refusal(N, B, D, C, flags, 7 | FRMAP_HEAD_FIT_EASY_MARGIN, required, 5,
                                "null pointer (x, labels, w, state and workspace are required)");
}

// The margin step (head_fit_rule.h, MARGIN): z by frmap_head_fit_dot, the norms and the float64 margin softmax of every counted row
// with serial sums, the figures, then the two chains over B, the combination and the update.  `given_g`: z, cosv, g, h, row_loss, rx
// and rw of the workspace are INPUTS (the device's own); row_src, n, the figures (the arg-max from the given z, rx and rw), dw and the
// update are computed from them.
inline const char* frmap_head_fit_margin_step_twin(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep,
                                                   float keep_scale, float* w, void* state, void* workspace, int N, int B, int D, int C,
                                                   const FrmapHeadFitMarginHyper& mh, const FrmapHeadFitHyper& h, int flags, int given_g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (const char* why = frmap_head_fit_margin_refusal(x, labels, w, state, workspace, N, B, D, C, flags)) return why;
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0, easy = (flags & FRMAP_HEAD_FIT_EASY_MARGIN) ? 1 : 0;
  const FrmapHeadFitState st = frmap_head_fit_state(state, D, C, amsgrad);
  const FrmapHeadFitMarginWork wk = frmap_head_fit_margin_work(workspace, B, C);
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
  if (!given_g) {
    for (int c = 0; c < C; ++c) {
      double sq = 0.0;
      for (int k = 0; k < D; ++k) sq = sq + (double)w[(size_t)c * (size_t)D + k] * (double)w[(size_t)c * (size_t)D + k];
      wk.rw[c] = frmap_head_fit_margin_rnorm(sq);
    }
  }
  const FrmapHeadFitTarget tg = frmap_head_fit_target(h.label_smoothing, C);
  uint64_t correct = 0, loss_q = 0;
  for (int i = 0; i < B; ++i) {
    const size_t at = (size_t)i * (size_t)C;
    float *z = wk.z + at, *cv = wk.cosv + at, *g = wk.g + at, *hh = wk.h + at;
    const int32_t r = wk.row_src[i];
    if (r < 0) {
      if (!given_g) {
        for (int c = 0; c < C; ++c) z[c] = cv[c] = g[c] = hh[c] = 0.0f;
        wk.row_loss[i] = __builtin_nanf("");
        wk.rx[i] = 0.0f;
      }
      continue;
    }
    const int32_t y = labels[r];
    if (!given_g) {
      double sq = 0.0;
      for (int k = 0; k < D; ++k) sq = sq + (double)xp(i, k) * (double)xp(i, k);
      wk.rx[i] = frmap_head_fit_margin_rnorm(sq);
      for (int c = 0; c < C; ++c) {
        const float* wc = w + (size_t)c * (size_t)D;
        z[c] = frmap_head_fit_dot(D, [&](int k) { return xp(i, k); }, [&](int k) { return wc[k]; });
      }
    }
    const float rxi = wk.rx[i];
    int inside_y;
    double out_y, dfac_y;
    const double cs_y = frmap_head_fit_margin_clamp(frmap_head_fit_margin_cos(z[y], rxi, wk.rw[y]), &inside_y);
    frmap_head_fit_margin_target(cs_y, inside_y, mh.m, easy, &out_y, &dfac_y);
    auto logit = [&](int c, double* cosine, int* inside) -> double {
      *cosine = frmap_head_fit_margin_cos(z[c], rxi, wk.rw[c]);
      return frmap_head_fit_margin_logit(frmap_head_fit_margin_clamp(*cosine, inside), c == y, out_y, mh.s);
    };
    double cosine, mx = -INFINITY;
    int inside, pred = 0x7FFFFFFF;
    for (int c = 0; c < C; ++c) {
      const double l = logit(c, &cosine, &inside);
      if (l > mx) { mx = l; pred = c; }
    }
    if (!given_g) {
      double sum = 0.0;
      for (int c = 0; c < C; ++c) sum = sum + exp(logit(c, &cosine, &inside) - mx);
      const double lse = log(sum);
      double nl_sum = 0.0;
      if (h.label_smoothing > 0.0f)
        for (int c = 0; c < C; ++c) nl_sum = nl_sum + (lse - (logit(c, &cosine, &inside) - mx));
      wk.row_loss[i] = frmap_head_fit_loss(lse - (logit(y, &cosine, &inside) - mx), nl_sum, h.label_smoothing, tg);
      for (int c = 0; c < C; ++c) {
        const double l = logit(c, &cosine, &inside);
        int in2;
        cv[c] = (float)frmap_head_fit_margin_clamp(cosine, &in2);
        frmap_head_fit_margin_gh(exp(l - mx), sum, c == y ? tg.y_on : tg.y_off, mh.s, n, c == y ? dfac_y : (inside ? 1.0 : 0.0), rxi, cosine, g + c,
                                 hh + c);
      }
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
  auto gg = [&](const float* m, int i, int c) -> float { return wk.row_src[i] < 0 ? 0.0f : m[(size_t)i * (size_t)C + c]; };
  for (int c = 0; c < C; ++c) {
    const float k = frmap_head_fit_dot(B, [&](int i) { return gg(wk.h, i, c); }, [](int) { return 1.0f; });
    for (int d = 0; d < D; ++d) {
      const float A = frmap_head_fit_dot(B, [&](int i) { return gg(wk.g, i, c); }, [&](int i) { return xp(i, d); });
      const size_t at = (size_t)c * (size_t)D + d;
      const float dw = frmap_head_fit_margin_dw(A, k, wk.rw[c], w[at]);
      frmap_head_fit_adam(a, dw, w + at, st.m_w + at, st.v_w + at, amsgrad ? st.vmax_w + at : nullptr);
    }
  }
  return nullptr;
}

// what an embedding call is refused for: the shared list (bit 16 of the flags is the easy margin), then what only it has
inline const char* frmap_head_fit_embed_refusal(const void* x, const void* labels, const void* w1, const void* gamma, const void* beta,
                                                const void* running_mean, const void* running_var, const void* wc, const void* state,
                                                const void* workspace, int N, int B, int D, int E, int C, int flags) {
  const void* const required[] = {x, labels, w1, gamma, beta, running_mean, running_var, wc, state, workspace};
  if (const char* why = frmap_head_fit_refusal(N, B, D, C, flags, 7 | FRMAP_HEAD_FIT_EASY_MARGIN, required, 10,
                                               "null pointer (x, labels, w1, gamma, beta, running_mean, running_var, wc, state and workspace are required)"))
    return why;
  if (E < 1 || E > FRMAP_HEAD_FIT_MAX_D) return "E is outside [1, 65536]";
  return nullptr;
}

// The embedding step (head_fit_rule.h, EMBED): layer 1 by frmap_head_fit_dot, the batch statistics with serial float64 sums, the margin
// twin on (y', lab) for the whole margin stage - on the real centres and their state, which are put back where the step is not taken -,
// then gy against the wc from BEFORE that update, the two chains over B, da and the updates.  `given` is a bit mask of the float64
// stages to take from the workspace as INPUTS (the device's own): 1 = mean32, rstd, uvar and ah; 2 = the margin stage, as the margin
// twin's given_g takes it; 4 = da.
inline const char* frmap_head_fit_embed_step_twin(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale,
                                                  float* w1, float* gamma, float* beta, float* running_mean, float* running_var, float* wc,
                                                  void* state, void* workspace, int N, int B, int D, int E, int C, const FrmapHeadFitBnHyper& bh,
                                                  const FrmapHeadFitMarginHyper& mh, const FrmapHeadFitHyper& h, int flags, int given) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const char* why = frmap_head_fit_embed_refusal(x, labels, w1, gamma, beta, running_mean, running_var, wc, state, workspace, N, B, D, E, C, flags);
  if (why) return why;
  if (given & ~7) return "given has unknown bits (1 statistics and ah, 2 the margin stage, 4 da)";
  const int amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0;
  const FrmapHeadFitEmbedState es = frmap_head_fit_embed_state(state, D, E, C, amsgrad);
  const FrmapHeadFitState st1 = frmap_head_fit_state(es.linear, D, E, amsgrad);
  const FrmapHeadFitState st2 = frmap_head_fit_state(es.bn, 1, E, amsgrad);
  const FrmapHeadFitState st3 = frmap_head_fit_state(es.margin, E, C, amsgrad);
  const FrmapHeadFitEmbedWork wk = frmap_head_fit_embed_work(workspace, B, E);
  const FrmapHeadFitMarginWork mw = frmap_head_fit_margin_work(wk.margin, B, C);
  uint64_t n1 = 0;
  for (int i = 0; i < B; ++i) {
    const int32_t r = wk.row_src1[i] = frmap_head_fit_row_src(x, labels, rows, i, N, D, C);
    wk.lab[i] = r < 0 ? -1 : labels[r];
    n1 += r >= 0 ? 1 : 0;
    float* ar = wk.a + (size_t)i * (size_t)E;
    for (int j = 0; j < E; ++j) {
      if (r < 0) {
        ar[j] = 0.0f;
        continue;
      }
      const float* xr = x + (size_t)r * (size_t)D;
      const float* wj = w1 + (size_t)j * (size_t)D;
      ar[j] = frmap_head_fit_dot(D, [&](int k) { return xr[k]; }, [&](int k) { return wj[k]; });
    }
  }
  wk.n1[0] = (int32_t)n1;
  wk.n1[1] = 0;
  const bool live = n1 >= 2;
  for (int j = 0; j < E; ++j) {
    if (!(given & 1)) {
      FrmapHeadFitBnStats bs = {0.0f, 0.0f, 0.0f};
      if (live) {
        double s = 0.0, q = 0.0;
        for (int i = 0; i < B; ++i)
          if (wk.row_src1[i] >= 0) s = s + (double)wk.a[(size_t)i * (size_t)E + j];
        const double mean = s / (double)n1;
        for (int i = 0; i < B; ++i) {
          if (wk.row_src1[i] < 0) continue;
          const double d = (double)wk.a[(size_t)i * (size_t)E + j] - mean;
          q = q + d * d;
        }
        bs = frmap_head_fit_bn_stats(mean, q, n1, bh.eps);
      }
      wk.mean32[j] = bs.mean32;
      wk.rstd[j] = bs.rstd;
      wk.uvar[j] = bs.uvar;
    }
    for (int i = 0; i < B; ++i) {
      const size_t at = (size_t)i * (size_t)E + j;
      const bool counted = live && wk.row_src1[i] >= 0;
      if (!(given & 1)) wk.ah[at] = counted ? frmap_head_fit_bn_ah(wk.a[at], wk.mean32[j], wk.rstd[j]) : 0.0f;
      wk.yp[at] = counted ? frmap_head_fit_bn_y(wk.ah[at], gamma[j], beta[j], keep ? (int)keep[at] : -1, keep_scale) : 0.0f;
    }
  }
  // the margin stage on the real centres and their state; both are put back where the step is not taken
  const size_t n_wc = (size_t)C * (size_t)E, n_st3 = frmap_head_fit_state_size(E, C, amsgrad);
  float* wc_old = new float[n_wc];
  unsigned char* st3_old = new unsigned char[n_st3];
  for (size_t k = 0; k < n_wc; ++k) wc_old[k] = wc[k];
  __builtin_memcpy(st3_old, es.margin, n_st3);
  why = frmap_head_fit_margin_step_twin(wk.yp, wk.lab, nullptr, nullptr, 1.0f, wc, es.margin, wk.margin, B, B, E, C, mh, h, flags, (given & 2) ? 1 : 0);
  if (why) {
    delete[] wc_old;
    delete[] st3_old;
    return why;
  }
  const uint64_t n2 = st3.head[FRMAP_HEAD_FIT_N];
  const bool taken = live && n2 == n1;
  if (!taken) {
    for (size_t k = 0; k < n_wc; ++k) wc[k] = wc_old[k];
    __builtin_memcpy(es.margin, st3_old, n_st3);
    if (flags & FRMAP_HEAD_FIT_CLEAR) st3.head[FRMAP_HEAD_FIT_ROWS] = st3.head[FRMAP_HEAD_FIT_CORRECT] = st3.head[FRMAP_HEAD_FIT_LOSS_Q] = 0;
    st3.head[FRMAP_HEAD_FIT_N] = 0;
  }
  delete[] st3_old;
  const uint64_t n = taken ? n1 : 0, t = st3.head[FRMAP_HEAD_FIT_T];
  st1.head[FRMAP_HEAD_FIT_T] = st2.head[FRMAP_HEAD_FIT_T] = t;
  st1.head[FRMAP_HEAD_FIT_N] = st2.head[FRMAP_HEAD_FIT_N] = n;
  st2.head[FRMAP_HEAD_FIT_ROWS] = st2.head[FRMAP_HEAD_FIT_CORRECT] = st2.head[FRMAP_HEAD_FIT_LOSS_Q] = 0;
  for (int i = 0; i < B; ++i) {
    const float* gr = mw.g + (size_t)i * (size_t)C;
    const float* hr = mw.h + (size_t)i * (size_t)C;
    const bool counted2 = mw.row_src[i] >= 0;
    const float k = frmap_head_fit_dot(C, [&](int c) { return hr[c]; }, [](int) { return 1.0f; });
    for (int e = 0; e < E; ++e) {
      const size_t at = (size_t)i * (size_t)E + e;
      const float S = frmap_head_fit_dot(C, [&](int c) { return gr[c] * mw.rw[c]; }, [&](int c) { return wc_old[(size_t)c * (size_t)E + e]; });
      wk.gy[at] = counted2 ? frmap_head_fit_embed_gy(S, k, mw.rx[i], wk.yp[at], keep ? (int)keep[at] : -1, keep_scale) : 0.0f;
    }
  }
  delete[] wc_old;
  const FrmapHeadFitAdam ad = frmap_head_fit_adam_scalars(t, h, flags);
  auto gyv = [&](int i, int j) -> float { return wk.row_src1[i] < 0 ? 0.0f : wk.gy[(size_t)i * (size_t)E + j]; };
  auto ahv = [&](int i, int j) -> float { return wk.row_src1[i] < 0 ? 0.0f : wk.ah[(size_t)i * (size_t)E + j]; };
  for (int j = 0; j < E; ++j) {
    const float db = wk.dbeta[j] = frmap_head_fit_dot(B, [&](int i) { return gyv(i, j); }, [](int) { return 1.0f; });
    const float dg = wk.dgamma[j] = frmap_head_fit_dot(B, [&](int i) { return gyv(i, j); }, [&](int i) { return ahv(i, j); });
    if (!(given & 4)) {
      for (int i = 0; i < B; ++i) {
        const size_t at = (size_t)i * (size_t)E + j;
        wk.da[at] = (n && wk.row_src1[i] >= 0) ? frmap_head_fit_bn_da(wk.gy[at], wk.ah[at], gamma[j], wk.rstd[j], db, dg, n) : 0.0f;
      }
    }
    if (!n) continue;
    frmap_head_fit_adam(ad, dg, gamma + j, st2.m_w + j, st2.v_w + j, amsgrad ? st2.vmax_w + j : nullptr);
    frmap_head_fit_adam(ad, db, beta + j, st2.m_b + j, st2.v_b + j, amsgrad ? st2.vmax_b + j : nullptr);
    running_mean[j] = frmap_head_fit_bn_running(running_mean[j], wk.mean32[j], bh.momentum);
    running_var[j] = frmap_head_fit_bn_running(running_var[j], wk.uvar[j], bh.momentum);
  }
  if (!n) return nullptr;
  auto dd = [&](int i, int j) -> float { return wk.row_src1[i] < 0 ? 0.0f : wk.da[(size_t)i * (size_t)E + j]; };
  for (int j = 0; j < E; ++j) {
    for (int d = 0; d < D; ++d) {
      const float dw = frmap_head_fit_dot(B, [&](int i) { return dd(i, j); }, [&](int i) { return wk.row_src1[i] < 0 ? 0.0f : x[(size_t)wk.row_src1[i] * (size_t)D + d]; });
      const size_t at = (size_t)j * (size_t)D + d;
      frmap_head_fit_adam(ad, dw, w1 + at, st1.m_w + at, st1.v_w + at, amsgrad ? st1.vmax_w + at : nullptr);
    }
  }
  return nullptr;
}
