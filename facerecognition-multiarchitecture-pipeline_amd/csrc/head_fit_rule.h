// One training step of a linear softmax classifier over cached features (head_fit.step_rule is the rule in plain numpy), for the
// host and the device alike: head_fit.hip's kernels and the host twin (head_fit_twin.h, frmap_head_fit_step_host) run this text; a
// plain C++ compiler takes it too (tools/head_fit_check.cpp).  Not part of the public ABI.
//
// Operands: x [N, D] fp32 (the cached features), labels [N] int32, rows [B] int32 (indices into x and labels; NULL: 0 .. B-1),
// keep [B, D] uint8 or NULL (a dropout mask over the BATCH rows), keep_scale = 1 / (1 - p), w [C, D] and b [C] fp32.
//   x'       = keep ? (keep[i][k] ? fl(x * keep_scale) : +0) : x                           one rounding
//   declined   batch row i is declined - it contributes nothing - when rows[i] is outside [0, N), or its label is outside [0, C),
//              or any of its D features is NaN or an infinity (the features themselves: a dropped one counts).  n = the batch
//              rows that are not declined.  n == 0: no weight, moment or step count changes; only the workspace is written.
//   z[i][c]  = dot_k(x'[i][k], w[c][k]) + b[c]                                              (declined: the row of z is +0)
//   softmax    in FLOAT64 from the fp32 logits: m = max_c z, s = sum_c exp(z - m), p = exp(z - m) / s, lse = log(s), -log p[c] =
//              lse - (z[c] - m); pred = the first arg-max
//   target     y_off = ls / C, y_on = (1 - ls) + y_off (ls == 0: exactly 0 and 1)
//   row loss = fp32(max(0, -log p[label])); with ls > 0: fp32(max(0, (1 - ls) (-log p[label]) + y_off sum_c (-log p[c])))
//              (declined: NaN)
//   g[i][c]  = fp32((p - y) / n)                                                             (declined: the row of g is +0)
//   dw[c][d] = dot_i(g[i][c], x'[i][d]), db[c] = dot_i(g[i][c], 1), declined rows taken as g = x' = +0
//   update     torch.optim.Adam / AdamW on every w[c][d] and b[c] (frmap_head_fit_adam below), t += 1 first
//   figures    rows += n, correct += #(pred == label), loss_q += the tally's fixed point of the row loss (tally_rule.h: clamp 65536,
//              scale 2^24): exact integer adds
//
// SUMMATION ORDER.  dot_k(a, b) over k = 0 .. K-1 (K = D forward, K = B backward) is cut at the multiples of FRMAP_HEAD_FIT_CHAIN:
//   s = +0;  for every chain j = 0, 1, ...: c = +0; for k = j CHAIN .. min((j + 1) CHAIN, K) - 1 ascending: c = fmaf(a_k, b_k, c);  s = s + c
// and the bias is added last, z = s + b.  Nothing depends on the grid, the device or the tiling: the fp32-input MFMA of gfx950 is
// bit for bit this fmaf chain over its two k, so a 32 x 32 tile on the matrix cores and a ragged edge on plain fmaf lanes agree.
// A chain never holds -0 (it starts at +0 and an exact zero sum rounds to +0), so a zero-padded k is a no-op.
// The softmax sums (s, and the smoothing sum) are float64 and the device's own: a wavefront adds them lane by lane and then across
// lanes, the twin serially, and exp / log are each side's library - parts in 2^53 before the one rounding to fp32, so g and the
// row loss of the two sides differ in a rare last bit at most.  Everything downstream of g is defined on g's fp32 bits.
//
// GROUPS (frmap_head_fit_group_step).  H independent heads over ONE cache: x and labels are shared; rows [H][B], keep [H][B][D],
// w [H][C][D], b [H][C], the states (frmap_head_fit_group_stride bytes apart: the single size rounded up to 8, so that every
// header stays 8-aligned; padding bytes are never touched) and the workspaces (back to back) are H single-head operands each.
// The scalars a single step takes by value are row h of hyper [H][8] fp32 in the memory the step runs on: lr, beta1, beta2, eps,
// weight_decay, label_smoothing, keep_scale, 0.  Head h of a grouped step has the bits of the single step on head h's slices.
// FRMAP_HEAD_FIT_EVAL (bit 8, groups only): logits, softmax and figures - n is written, rows / correct / loss_q are added to - and
// nothing else: t, the weights and the moments stay.
//
// STATE (frmap_head_fit_state_bytes; all-zero bytes = fresh): eight uint64 words - t, n of the step in flight, and the epoch figures
// rows, correct, loss_q, three reserved - then fp32 m_w [C D], v_w [C D], m_b [C], v_b [C] and, with AMSGrad, vmax_w [C D], vmax_b [C].
// WORKSPACE (frmap_head_fit_workspace_bytes): fp32 z [B C], g [B C], row_loss [B], then int32 row_src [B]: the row of x a batch row
// reads, or -1 for a declined one.
//
// HIDDEN LAYER (frmap_head_fit_hidden_step; head_fit.hidden_step_rule in numpy).  Linear(D, Hd) -> ReLU -> dropout -> Linear(Hd, C): plain
// backpropagation through one ReLU.  x, labels and rows are the linear step's; keep1 [B, D] / keep1_scale mask the input, keep2 [B, Hd] /
// keep2_scale the hidden layer; the parameters are w1 [Hd, D], b1 [Hd], w2 [C, Hd], b2 [C].
//   x'       = frmap_head_fit_xp(x, keep1, keep1_scale)
//   a[i][j]  = dot_k(x'[i][k], w1[j][k]) + b1[j]                              chain order over D, bias last
//   h[i][j]  = a > 0 ? a : (a != a ? a : +0)                                  a NaN stays one; -0 and negatives give +0
//   lab[i]   = labels[rows[i]], or -1 where layer 1 declines row i (row index outside [0, N), label outside [0, C), a non-finite
//              feature); the h row of such a row is +0.  row_src1[i] is the row of x read, or -1.
//   layer 2  = the linear step's forward half on (x := h [B, Hd], labels := lab [B], rows := NULL, keep := keep2, w2, b2):
//              h' = xp(h, keep2, keep2_scale), z, the float64 softmax, the row loss, g = (p - y) / n, the figures.  It declines a row
//              whose lab is -1 or whose h holds a non-finite value.  n is ITS count: the one n of the step.
//   s[i][j]  = dot_c(g[i][c], w2[c][j])                                       chain order over C, w2 BEFORE its update
//   da[i][j] = (row i counted by layer 2) && h[i][j] > 0 && kept2[i][j] ? fl(s * keep2_scale) : +0      (no mask: s itself)
//   dw2, db2 = the linear step's on (g, h');  dw1[j][d] = dot_i(da[i][j], x'[i][d]), db1[j] = dot_i(da[i][j], 1), the rows that
//              layer 1 declined taken as da = x' = +0
//   update   = frmap_head_fit_adam on all four with the same hyper-parameters and the same t (one optimiser over four tensors).
//              n == 0: nothing changes but the workspace.
// HIDDEN STATE (frmap_head_fit_hidden_state_bytes): the single layout for (D, Hd), then the single layout for (Hd, C); both are
// multiples of 8 and all-zero bytes are a fresh state.  The second part is a valid state of the linear step on (h, lab): its header
// carries t, n and the epoch figures.  The first part's t and n are copies written by the step; its figure words stay 0.
// HIDDEN WORKSPACE (frmap_head_fit_hidden_workspace_bytes): fp32 h [B Hd], da [B Hd], int32 lab [B], row_src1 [B], then the single
// workspace for (B, Hd -> C).
//
// PAIR (frmap_head_fit_pair_step; head_fit.pair_step_rule in numpy).  A contrastive head x -> normalize(x w^T + b) over PAIRS of cached
// rows: left [P], right [P] int32 rows of x, differ [P] int32 (0: the same identity, pulled together; 1: different, pushed apart up
// to `margin`), keep [2P, D] uint8 or NULL with keep_scale, w [E, D], b [E], the floats margin, w_same, w_diff, accept.
//   batch      2P rows: row i < P reads left[i], row P + i reads right[i].  A row is declined when its index is outside [0, N) or
//              any of its D features is non-finite (no label is read).
//   a[i][e]  = dot_k(x'[i][k], w[e][k]) + b[e]                          chain order over D, bias last; a declined row is +0
//   counted    pair p is counted iff both of its rows are and differ[p] is 0 or 1; n = the counted pairs.  An uncounted pair has
//              row_src = -1 on BOTH its rows, +0 rows of ga, NaN in pair_loss and dist.  n == 0: nothing changes but the workspace.
//   loss       per counted pair in FLOAT64 from the fp32 a, rounded to fp32 once (the stance of the softmax half):
//              s = max(||a||, 1e-12), u = a_l / s_l, v = a_r / s_r                 (F.normalize)
//              delta = (u - v) + 1e-6, d0 = ||delta||, d = max(d0, 1e-8)           (F.pairwise_distance, then the clamp)
//              pair_loss = differ ? w_diff max(margin - d, 0)^2 : w_same d^2;  dist = d
//              q = (differ ? -2 w_diff max(margin - d, 0) : 2 w_same d) / n, 0 where d0 < 1e-8;  gd = q delta / d0
//              ga_l = (gd - u (u . gd)) / s_l where ||a_l|| > 1e-12, else gd / 1e-12;  ga_r the same with -gd and v
//   figures    rows += n, correct += #((dist < accept) == (differ == 0)) on the fp32 dist, loss_q += the fixed point of pair_loss
//   update     the linear step's on (x, keep, g := ga, row_src) with B := 2P, C := E: dw = ga^T x', db = sum ga, Adam, t += 1 first
// The float64 sums (||a||^2 of both rows, then ||delta||^2, u . delta, v . delta) are each side's own order, as the softmax sums are:
// parts in 2^53 before the one rounding, so ga, pair_loss and dist of the two sides differ in a rare last bit at most.  Everything
// downstream of ga is defined on ga's fp32 bits.
// PAIR STATE: the single layout for (D, E).  PAIR WORKSPACE (frmap_head_fit_pair_workspace_bytes): fp32 a [2P E], ga [2P E],
// pair_loss [P], dist [P], then int32 row_src [2P].
//
// MARGIN (frmap_head_fit_margin_step; head_fit.margin_step_rule in numpy).  The class centres w [C, D] of an ArcFace margin head
// (the reference's ArcMarginProduct, src/face_models.py:297-429) under softmax cross-entropy: x, labels, rows, keep / keep_scale and the
// declined rows are the linear step's; there is NO bias.  The scalars are s (the effective scale), m (the effective margin: the
// schedule that produces them is host code, head_fit.margin_schedule), ls and the Adam scalars; FRMAP_HEAD_FIT_EASY_MARGIN (bit 16 of
// `flags`) selects the easy margin.
//   z[i][c]  = dot_k(x'[i][k], w[c][k])                                 chain order over D, no bias; a declined row is +0
//   rx[i]    = fp32(1 / max(||x'_i||, 1e-12)), rw[c] = fp32(1 / max(||w_c||, 1e-12)): the squared norms are FLOAT64 sums of the fp32
//              elements (each side's own order), the reciprocal rounded to fp32 once; rx of a declined row is +0.  Everything below
//              is defined on the fp32 bits of z, rx and rw, in FLOAT64 up to the one rounding of cosv, g, h and the row loss.
//   cos      = (z rx[i]) rw[c];  cs = clamp(cos, LO, HI), inside = LO <= cos <= HI, with LO, HI the fp32 roundings of -+(1 - 1e-7)
//   target y : theta = acos(cs);  standard: theta + m >= CAP ? (out = cos(CAP), dfac = 0)
//                                                            : (out = cos(theta + m), dfac = inside sin(theta + m) / sin(theta)), CAP the
//              fp32 value of pi - 1e-4 (a NaN is not capped and stays one);
//              easy margin: cs > 0 ? (out = cos(theta + m), dfac as above) : (out = cs, dfac = inside).  Others: out = cs, dfac = inside.
//   l        = s out;  pred = the first arg-max of l;  softmax, -log p and the row loss from l as the linear step forms them from z
//   q        = (s (p - y)) / n;  gcos = q dfac;  g[i][c] = fp32(gcos rx[i]), h[i][c] = fp32(gcos cos)      (declined: +0 rows)
//   cosv     = fp32(cs)                                                  (for inspection; nothing reads it)
//   dw[c][d] = fl(fl(rw[c] A) - fl(fl(fl(rw[c] rw[c]) k[c]) w[c][d])), A = dot_i(g[i][c], x'[i][d]), k[c] = dot_i(h[i][c], 1); the
//              second term is absent where rw[c] is not below fp32(1e12), the reciprocal of the clamped norm (torch's clamp_min passes
//              no gradient there)
//   update     frmap_head_fit_adam on every w[c][d], t += 1 first; figures as in the linear step.  n == 0: only the workspace is written.
// MARGIN STATE: the single layout for (D, C); the bias moments stay zero.  MARGIN WORKSPACE (frmap_head_fit_margin_workspace_bytes):
// fp32 z [B C], cosv [B C], g [B C], h [B C], row_loss [B], rx [B], rw [C], then int32 row_src [B].
//
// EMBED (frmap_head_fit_embed_step; head_fit.embed_step_rule in numpy).  The embedding layer of an ArcFace model with the trunk frozen,
// x -> x w1^T -> BatchNorm1d in TRAINING mode -> dropout -> F.normalize -> ArcMarginProduct -> cross-entropy (the first phase of the
// reference's two-phase training, src/training.py:374-377, 683-700, src/face_models.py:492-498, 511-535), over cached POOLED trunk
// features: x, labels and rows are the linear step's; keep [B, E] / keep_scale is the dropout BEHIND the BatchNorm (the reference's
// position); the parameters are w1 [E, D] (no bias), gamma, beta, running_mean, running_var [E] and the class centres wc [C, E]; the
// scalars bn_eps, bn_momentum, s, m, ls and the Adam scalars; flags 1 | 2 | 4 | 16 with the margin step's meaning.
//   declined   layer 1 declines batch row i as the linear step does (row index, label outside [0, C), a non-finite feature):
//              lab[i] = -1 and row_src1[i] = -1, else the label and the row of x.  n1 = the rows that remain.
//   a[i][j]  = dot_k(x[i][k], w1[j][k])                                  chain order over D, no bias; a declined row is +0
//   batch statistics, per column j over the n1 counted rows, in FLOAT64 from the fp32 a (each side's own summation order):
//              mean = (sum_i a) / n1;  var = (sum_i (a - mean)^2) / n1, the second pass against the float64 mean;
//              mean32 = fp32(mean), rstd = fp32(1 / sqrt(var + bn_eps)), uvar = fp32((var n1) / (n1 - 1)): one rounding each.
//              n1 < 2: no statistic exists (torch refuses one value per channel); mean32 = rstd = uvar = +0 and every ah, y' is +0.
//   ah[i][j] = fp32(((double)a - (double)mean32) (double)rstd)            float64 on the fp32 bits, one rounding
//   y[i][j]  = fl(fl(gamma[j] ah) + beta[j]);  y' = kept ? fl(y keep_scale) : +0 (no mask: y);  declined rows of ah and y' are +0
//   margin   = the margin step's forward half on (x := y' [B, E], labels := lab [B], rows := NULL, keep := NULL, w := wc): z, rx,
//              rw, cosv, g, h, row_loss and the figures of the step are frmap_head_fit_margin_step's on those operands, bit for bit.
//              Its count is n2; it declines a row whose lab is -1 or whose y' holds a non-finite value; its g and h carry 1 / n2.
//   taken      the step is TAKEN iff n1 >= 2 and n2 == n1 (all or nothing: a non-finite y' has poisoned a whole column).  A step that
//              is not taken writes the workspace and nothing else: no parameter, moment, running statistic, epoch figure or t moves;
//              the word n of the three headers is 0 after it.  CHOSEN HERE: bit 4 (clear) zeroes the epoch figures either way, as
//              the caller asked; da of a step that is not taken is all +0; gy, dbeta and dgamma are still written.
//   gy'[i][e]= fl(S - fl(fl(fl(rx_i rx_i) k_i) y'[i][e])),  S = dot_c(gw[i][c], wc[c][e]) chained over C with gw = fl(g[i][c] rw[c])
//              and wc BEFORE its update, k_i = dot_c(h[i][c], 1) chained over C; the second term is absent where rx_i is not below
//              fp32(1e12) (the mirror of frmap_head_fit_margin_dw).  gy = kept ? fl(gy' keep_scale) : +0 (no mask: gy').
//              CHOSEN HERE: a row the margin stage did not count has gy = +0, and gy (after the gate) is what the workspace keeps.
//   dbeta[j] = dot_i(gy[i][j], 1), dgamma[j] = dot_i(gy[i][j], ah[i][j])   chain order over B, rows declined by layer 1 taken as +0
//   da[i][j] = fp32((gamma_j rstd_j) ((gy - dbeta_j / n1) - ah (dgamma_j / n1)))   float64 on the fp32 bits in exactly this
//              association (frmap_head_fit_bn_da), gamma BEFORE its update; declined rows are +0
//   dw1[j][d]= dot_i(da[i][j], x[i][d]);  dwc = the margin step's own on (y', g, h, rw)
//   update     frmap_head_fit_adam on w1, gamma (gradient dgamma), beta (gradient dbeta) and wc with the same hyper-parameters and
//              the same t: one optimiser over four tensors, weight decay on all four as the reference's one parameter group has it.
//              running_mean = fl(fl(fl(1 - mom) rm) + fl(mom mean32)); running_var likewise with uvar.
// EMBED STATE (frmap_head_fit_embed_state_bytes; all-zero bytes = fresh): three single layouts back to back, each a multiple of 8 -
// (D, E) for w1 (its bias moments stay zero), (1, E) for gamma as the "weight" and beta as the "bias", and (E, C), a valid MARGIN
// STATE of the centres whose header carries t, n and the epoch figures.  The first two headers carry copies of t and n; the second
// one also serves the margin forward half as the header of the step in flight and has zero figure words between steps.
// EMBED WORKSPACE (frmap_head_fit_embed_workspace_bytes): fp32 a, ah, y', gy, da [B E], mean32, rstd, uvar, dbeta, dgamma [E], int32
// lab [B], row_src1 [B], n1 and one padding word, then the margin workspace for (B, C).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "tally_rule.h"   // FRMAP_TRACK_HD, frmap_tally_finite_bits, frmap_tally_loss_q

constexpr int FRMAP_HEAD_FIT_CHAIN = 128;
constexpr int FRMAP_HEAD_FIT_MAX_C = 65536;              // classes (the softmax kernel gives a wavefront to a row; the grid of the update)
constexpr int FRMAP_HEAD_FIT_MAX_D = 65536;
constexpr int FRMAP_HEAD_FIT_MAX_B = 1 << 20;            // batch rows of one step
constexpr int FRMAP_HEAD_FIT_DECOUPLED = 1, FRMAP_HEAD_FIT_AMSGRAD = 2, FRMAP_HEAD_FIT_CLEAR = 4;   // bits of `flags`
constexpr int FRMAP_HEAD_FIT_HEADER = 8;
constexpr int FRMAP_HEAD_FIT_T = 0, FRMAP_HEAD_FIT_N = 1, FRMAP_HEAD_FIT_ROWS = 2, FRMAP_HEAD_FIT_CORRECT = 3, FRMAP_HEAD_FIT_LOSS_Q = 4;

FRMAP_TRACK_HD inline bool frmap_head_fit_shape_ok(int D, int C) {
  return D >= 1 && D <= FRMAP_HEAD_FIT_MAX_D && C >= 1 && C <= FRMAP_HEAD_FIT_MAX_C;
}
FRMAP_TRACK_HD inline size_t frmap_head_fit_state_size(int D, int C, int amsgrad) {
  const size_t per = (size_t)C * (size_t)D + (size_t)C;
  return (((size_t)FRMAP_HEAD_FIT_HEADER * 8 + 4 * per * (amsgrad ? 3 : 2)) + 7) & ~(size_t)7;
}
FRMAP_TRACK_HD inline size_t frmap_head_fit_workspace_size(int B, int C) { return 4 * (2 * (size_t)B * (size_t)C + 2 * (size_t)B); }

// groups of heads (the comment at the top, GROUPS)
constexpr int FRMAP_HEAD_FIT_EVAL = 8;                   // bit of `flags`, grouped step only
constexpr int FRMAP_HEAD_FIT_MAX_H = 4096;
constexpr int FRMAP_HEAD_FIT_HYPER_COLS = 8;             // lr, beta1, beta2, eps, weight_decay, label_smoothing, keep_scale, 0
constexpr int FRMAP_HEAD_FIT_HYPER_KEEP_SCALE = 6;
static_assert(sizeof(size_t) == 8, "the offsets of a group are size_t products of h, the stride and the extents: 64 bits");
FRMAP_TRACK_HD inline size_t frmap_head_fit_group_stride(int D, int C, int amsgrad) {
  return (frmap_head_fit_state_size(D, C, amsgrad) + 7) & ~(size_t)7;
}
// whether every byte count of a group (the states, the workspaces, w, keep) is a product that 64 bits hold
inline bool frmap_head_fit_group_fits(int H, int B, int D, int C, int amsgrad) {
  unsigned long long states = 0, works = 0, wb = 0, kb = 0, bd = 0;
  if (__builtin_mul_overflow((unsigned long long)H, (unsigned long long)frmap_head_fit_group_stride(D, C, amsgrad), &states)) return false;
  if (__builtin_mul_overflow((unsigned long long)H, (unsigned long long)frmap_head_fit_workspace_size(B, C), &works)) return false;
  if (__builtin_mul_overflow((unsigned long long)H * 4ull, (unsigned long long)C * (unsigned long long)D, &wb)) return false;
  if (__builtin_mul_overflow((unsigned long long)B, (unsigned long long)D, &bd) || __builtin_mul_overflow((unsigned long long)H, bd, &kb)) return false;
  return true;
}

struct FrmapHeadFitState {
  uint64_t* head;
  float *m_w, *v_w, *m_b, *v_b, *vmax_w, *vmax_b;
};
FRMAP_TRACK_HD inline FrmapHeadFitState frmap_head_fit_state(void* state, int D, int C, int amsgrad) {
  FrmapHeadFitState s;
  const size_t cd = (size_t)C * (size_t)D;
  s.head = (uint64_t*)state;
  s.m_w = (float*)(s.head + FRMAP_HEAD_FIT_HEADER);
  s.v_w = s.m_w + cd;
  s.m_b = s.v_w + cd;
  s.v_b = s.m_b + C;
  s.vmax_w = amsgrad ? s.v_b + C : nullptr;
  s.vmax_b = amsgrad ? s.vmax_w + cd : nullptr;
  return s;
}
struct FrmapHeadFitWork {
  float *z, *g, *row_loss;
  int32_t* row_src;
};
FRMAP_TRACK_HD inline FrmapHeadFitWork frmap_head_fit_work(void* workspace, int B, int C) {
  FrmapHeadFitWork k;
  k.z = (float*)workspace;
  k.g = k.z + (size_t)B * (size_t)C;
  k.row_loss = k.g + (size_t)B * (size_t)C;
  k.row_src = (int32_t*)(k.row_loss + B);
  return k;
}

struct FrmapHeadFitHyper {
  float lr, beta1, beta2, eps, weight_decay, label_smoothing;
};

// x' of one feature; `kept` < 0: no mask
FRMAP_TRACK_HD inline float frmap_head_fit_xp(float x, int kept, float keep_scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (kept < 0) return x;
  return kept ? x * keep_scale : 0.0f;
}

// The softmax half of a row, in FLOAT64 from the fp32 logits and rounded to fp32 once at the end: g and the row loss are then
// within one fp32 unit in the last place of their exact values whatever library evaluates exp and log, and the order of the two
// sums moves them by parts in 2^53.
struct FrmapHeadFitTarget {
  double y_on, y_off, one_minus_ls;
};
FRMAP_TRACK_HD inline FrmapHeadFitTarget frmap_head_fit_target(float ls, int C) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  FrmapHeadFitTarget t;
  t.one_minus_ls = 1.0 - (double)ls;
  t.y_off = ls > 0.0f ? (double)ls / (double)C : 0.0;
  t.y_on = t.one_minus_ls + t.y_off;
  return t;
}
// exp(z - m) of one logit against the row maximum
FRMAP_TRACK_HD inline double frmap_head_fit_exp(float z, float m) { return exp((double)z - (double)m); }
// -log p of one class: lse - (z - m) with lse = log(sum_c exp(z[c] - m))
FRMAP_TRACK_HD inline double frmap_head_fit_nl(double lse, float z, float m) { return lse - ((double)z - (double)m); }
// the row loss from -log p of the label and, with smoothing, the sum over the classes of -log p
FRMAP_TRACK_HD inline float frmap_head_fit_loss(double nl_label, double nl_sum, float ls, const FrmapHeadFitTarget& t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double l = nl_label;
  if (ls > 0.0f) {
    const double a = t.one_minus_ls * nl_label, b = t.y_off * nl_sum;
    l = a + b;
  }
  return (float)(l > 0.0 ? l : (l == l ? 0.0 : l));       // max(0, l); a NaN stays one
}
FRMAP_TRACK_HD inline float frmap_head_fit_g(double e, double s, double y, uint64_t n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double p = e / s;
  const double d = p - y;
  return (float)(d / (double)n);
}

// The scalars of step t (the count AFTER its increment) that every element shares.  beta^t is a product of squarings in double, so
// the host and the device form the same bits; the corrections are rounded to fp32 once.
struct FrmapHeadFitAdam {
  float step_size, bc2_sqrt, omb1, omb2, beta2, eps, wd, decay;
  int decoupled, amsgrad;
};
FRMAP_TRACK_HD inline double frmap_head_fit_powi(double base, uint64_t t) {
  double r = 1.0, p = base;
  while (t) {
    if (t & 1) r = r * p;
    p = p * p;
    t >>= 1;
  }
  return r;
}
FRMAP_TRACK_HD inline FrmapHeadFitAdam frmap_head_fit_adam_scalars(uint64_t t, const FrmapHeadFitHyper& h, int flags) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  FrmapHeadFitAdam a;
  const float bc1 = (float)(1.0 - frmap_head_fit_powi((double)h.beta1, t));
  const float bc2 = (float)(1.0 - frmap_head_fit_powi((double)h.beta2, t));
  a.step_size = h.lr / bc1;
  a.bc2_sqrt = sqrtf(bc2);
  a.omb1 = 1.0f - h.beta1;
  a.omb2 = 1.0f - h.beta2;
  a.beta2 = h.beta2;
  a.eps = h.eps;
  a.wd = h.weight_decay;
  const float lw = h.lr * h.weight_decay;
  a.decay = 1.0f - lw;
  a.decoupled = (flags & FRMAP_HEAD_FIT_DECOUPLED) ? 1 : 0;
  a.amsgrad = (flags & FRMAP_HEAD_FIT_AMSGRAD) ? 1 : 0;
  return a;
}
// torch.optim.Adam / AdamW on one parameter with gradient `grad`, every operation fp32 and rounded once:
//   coupled    grad = fma(wd, p, grad)                         decoupled   p = p * (1 - lr wd)
//   m = fma(1 - beta1, grad - m, m)                            (exp_avg.lerp_)
//   v = fma(1 - beta2, grad * grad, v * beta2)                 (mul_ then addcmul_)
//   vhat = amsgrad ? (vmax = max(vmax, v)) : v
//   p = fma(-step_size, m / (sqrt(vhat) / sqrt(1 - beta2^t) + eps), p),  step_size = lr / (1 - beta1^t)
FRMAP_TRACK_HD inline void frmap_head_fit_adam(const FrmapHeadFitAdam& a, float grad, float* p_io, float* m_io, float* v_io, float* vmax_io) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float p = *p_io, m = *m_io, v = *v_io;
  if (a.decoupled) {
    p = p * a.decay;
  } else if (a.wd != 0.0f) {
    grad = fmaf(a.wd, p, grad);
  }
  const float diff = grad - m;
  m = fmaf(a.omb1, diff, m);
  const float vb = v * a.beta2;
  const float gg = grad * grad;
  v = fmaf(a.omb2, gg, vb);
  float vhat = v;
  if (a.amsgrad) {
    const float old = *vmax_io;
    vhat = old > v ? old : v;
    *vmax_io = vhat;
  }
  const float r = sqrtf(vhat);
  const float q = r / a.bc2_sqrt;
  const float denom = q + a.eps;
  const float u = m / denom;
  p = fmaf(-a.step_size, u, p);
  *p_io = p;
  *m_io = m;
  *v_io = v;
}

// the hidden-layer step (the comment at the top, HIDDEN LAYER)
FRMAP_TRACK_HD inline bool frmap_head_fit_hidden_shape_ok(int D, int Hd, int C) {
  return frmap_head_fit_shape_ok(D, Hd) && frmap_head_fit_shape_ok(Hd, C);
}
FRMAP_TRACK_HD inline size_t frmap_head_fit_hidden_state_size(int D, int Hd, int C, int amsgrad) {
  return frmap_head_fit_state_size(D, Hd, amsgrad) + frmap_head_fit_state_size(Hd, C, amsgrad);
}
FRMAP_TRACK_HD inline size_t frmap_head_fit_hidden_workspace_size(int B, int Hd, int C) {
  return 4 * (2 * (size_t)B * (size_t)Hd + 2 * (size_t)B) + frmap_head_fit_workspace_size(B, C);
}
struct FrmapHeadFitHiddenWork {
  float *h, *da;
  int32_t *lab, *row_src1;
  void* layer2;              // the single workspace for (B, Hd -> C)
};
FRMAP_TRACK_HD inline FrmapHeadFitHiddenWork frmap_head_fit_hidden_work(void* workspace, int B, int Hd) {
  FrmapHeadFitHiddenWork k;
  k.h = (float*)workspace;
  k.da = k.h + (size_t)B * (size_t)Hd;
  k.lab = (int32_t*)(k.da + (size_t)B * (size_t)Hd);
  k.row_src1 = k.lab + B;
  k.layer2 = (void*)(k.row_src1 + B);
  return k;
}
// h of one pre-activation: a NaN stays one; -0 and negatives give +0
FRMAP_TRACK_HD inline float frmap_head_fit_relu(float a) { return a > 0.0f ? a : (a != a ? a : 0.0f); }
// da of one hidden unit from s = dot_c(g, w2); `kept` < 0: no mask
FRMAP_TRACK_HD inline float frmap_head_fit_da(float s, float h, int kept, float keep_scale, bool counted) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!counted || !(h > 0.0f) || kept == 0) return 0.0f;
  return kept < 0 ? s : s * keep_scale;
}

// the pair step (the comment at the top, PAIR)
constexpr int FRMAP_HEAD_FIT_MAX_P = FRMAP_HEAD_FIT_MAX_B / 2;      // pairs of one step: 2P batch rows
FRMAP_TRACK_HD inline bool frmap_head_fit_pair_shape_ok(int P, int D, int E) {
  return frmap_head_fit_shape_ok(D, E) && P >= 1 && P <= FRMAP_HEAD_FIT_MAX_P;
}
FRMAP_TRACK_HD inline size_t frmap_head_fit_pair_workspace_size(int P, int E) {
  return 4 * (4 * (size_t)P * (size_t)E + 4 * (size_t)P);
}
struct FrmapHeadFitPairWork {
  float *a, *ga, *pair_loss, *dist;
  int32_t* row_src;
};
FRMAP_TRACK_HD inline FrmapHeadFitPairWork frmap_head_fit_pair_work(void* workspace, int P, int E) {
  FrmapHeadFitPairWork k;
  const size_t pe2 = 2 * (size_t)P * (size_t)E;
  k.a = (float*)workspace;
  k.ga = k.a + pe2;
  k.pair_loss = k.ga + pe2;
  k.dist = k.pair_loss + P;
  k.row_src = (int32_t*)(k.dist + P);
  return k;
}
struct FrmapHeadFitPairHyper {
  float margin, w_same, w_diff, accept;
};
// delta of one element from the two rows' values and norms, with u and v
FRMAP_TRACK_HD inline double frmap_head_fit_pair_delta(float al, float ar, double sl, double sr, double* u, double* v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *u = (double)al / sl;
  *v = (double)ar / sr;
  const double uv = *u - *v;
  return uv + 1e-6;
}
// What the elements of a pair share, from the five float64 sums: nl2 = sum a_l^2, nr2 = sum a_r^2, dd = sum delta^2, ud = u . delta,
// vd = v . delta.  ga_l[e] = cl (delta - u ud) (or cl delta where ||a_l|| <= 1e-12: cl then carries 1 / 1e-12), ga_r[e] = cr (delta - v vd).
struct FrmapHeadFitPair {
  double sl, sr, ud, vd, cl, cr;
  int l_free, r_free;        // the row's norm is above 1e-12: the normalisation has a gradient of its own
  float loss, dist;
};
FRMAP_TRACK_HD inline void frmap_head_fit_pair_norms(double nl2, double nr2, FrmapHeadFitPair* p) {
  const double l = sqrt(nl2), r = sqrt(nr2);
  p->l_free = l > 1e-12 ? 1 : 0;
  p->r_free = r > 1e-12 ? 1 : 0;
  p->sl = l > 1e-12 ? l : (l == l ? 1e-12 : l);              // max(l, 1e-12); a NaN stays one
  p->sr = r > 1e-12 ? r : (r == r ? 1e-12 : r);
}
FRMAP_TRACK_HD inline void frmap_head_fit_pair_scalars(double dd, double ud, double vd, int differ, uint64_t n, const FrmapHeadFitPairHyper& h,
                                                       FrmapHeadFitPair* p) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d0 = sqrt(dd);
  const double d = d0 > 1e-8 ? d0 : (d0 == d0 ? 1e-8 : d0);
  double loss, q;
  if (differ) {
    const double gap = (double)h.margin - d;
    const double m = gap > 0.0 ? gap : (gap == gap ? 0.0 : gap);
    loss = (double)h.w_diff * (m * m);
    q = -2.0 * (double)h.w_diff * m;
  } else {
    loss = (double)h.w_same * (d * d);
    q = 2.0 * (double)h.w_same * d;
  }
  q = q / (double)n;
  const double c = d0 < 1e-8 ? 0.0 : q / d0;
  p->ud = ud;
  p->vd = vd;
  p->cl = c / p->sl;
  p->cr = -c / p->sr;
  p->loss = (float)loss;
  p->dist = (float)d;
}
FRMAP_TRACK_HD inline void frmap_head_fit_pair_ga(float al, float ar, const FrmapHeadFitPair& p, float* gl, float* gr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double u, v;
  const double delta = frmap_head_fit_pair_delta(al, ar, p.sl, p.sr, &u, &v);
  const double tl = p.l_free ? delta - u * p.ud : delta;
  const double tr = p.r_free ? delta - v * p.vd : delta;
  *gl = (float)(p.cl * tl);
  *gr = (float)(p.cr * tr);
}

// the margin step (the comment at the top, MARGIN)
constexpr int FRMAP_HEAD_FIT_EASY_MARGIN = 16;           // bit of `flags`, margin step only
constexpr float FRMAP_HEAD_FIT_MARGIN_HI = (float)(1.0 - 1e-7);                  // the clamp bound of the cosine, as fp32
constexpr float FRMAP_HEAD_FIT_MARGIN_CAP = (float)(3.14159265358979323846 - 1e-4);   // the largest theta + m, as fp32
constexpr float FRMAP_HEAD_FIT_MARGIN_RMAX = (float)(1.0 / 1e-12);               // the reciprocal of a clamped norm
FRMAP_TRACK_HD inline size_t frmap_head_fit_margin_workspace_size(int B, int C) {
  return 4 * (4 * (size_t)B * (size_t)C + 3 * (size_t)B + (size_t)C);
}
struct FrmapHeadFitMarginWork {
  float *z, *cosv, *g, *h, *row_loss, *rx, *rw;
  int32_t* row_src;
};
FRMAP_TRACK_HD inline FrmapHeadFitMarginWork frmap_head_fit_margin_work(void* workspace, int B, int C) {
  FrmapHeadFitMarginWork k;
  const size_t bc = (size_t)B * (size_t)C;
  k.z = (float*)workspace;
  k.cosv = k.z + bc;
  k.g = k.cosv + bc;
  k.h = k.g + bc;
  k.row_loss = k.h + bc;
  k.rx = k.row_loss + B;
  k.rw = k.rx + B;
  k.row_src = (int32_t*)(k.rw + C);
  return k;
}
// 1 / max(sqrt(sq), 1e-12) from the float64 sum of squares of a row, rounded to fp32 once
FRMAP_TRACK_HD inline float frmap_head_fit_margin_rnorm(double sq) {
  const double r = sqrt(sq);
  return (float)(1.0 / (r > 1e-12 ? r : (r == r ? 1e-12 : r)));
}
// the cosine of one element before the clamp
FRMAP_TRACK_HD inline double frmap_head_fit_margin_cos(float z, float rx, float rw) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double a = (double)z * (double)rx;
  return a * (double)rw;
}
// the clamped cosine; *inside: the clamp passes a gradient (bounds included).  A NaN stays one, outside.
FRMAP_TRACK_HD inline double frmap_head_fit_margin_clamp(double c, int* inside) {
  const double hi = (double)FRMAP_HEAD_FIT_MARGIN_HI, lo = -hi;
  *inside = (c >= lo && c <= hi) ? 1 : 0;
  return c < lo ? lo : (c > hi ? hi : c);
}
// out and dfac of the TARGET element of a row from its clamped cosine
FRMAP_TRACK_HD inline void frmap_head_fit_margin_target(double cs, int inside, float m, int easy, double* out, double* dfac) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double in = inside ? 1.0 : 0.0;
  if (easy && !(cs > 0.0)) {
    *out = cs;
    *dfac = in;
    return;
  }
  const double theta = acos(cs);
  const double tm = theta + (double)m;
  if (!easy && tm >= (double)FRMAP_HEAD_FIT_MARGIN_CAP) {                // (a NaN is not capped: it stays one, as torch.minimum keeps it)
    *out = cos((double)FRMAP_HEAD_FIT_MARGIN_CAP);
    *dfac = 0.0;
    return;
  }
  *out = cos(tm);
  const double ratio = sin(tm) / sin(theta);
  *dfac = in * ratio;
}
// the logit of one element: the target's `out_y`, else the clamped cosine, times s
FRMAP_TRACK_HD inline double frmap_head_fit_margin_logit(double cs, bool target, double out_y, float s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (double)s * (target ? out_y : cs);
}
// g and h of one element: e = exp(l - max), sum = the row's sum of them, y the smoothed target, dfac the element's
FRMAP_TRACK_HD inline void frmap_head_fit_margin_gh(double e, double sum, double y, float s, uint64_t n, double dfac, float rx, double cosine,
                                                    float* g, float* h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double p = e / sum;
  const double d = p - y;
  const double sd = (double)s * d;
  const double q = sd / (double)n;
  const double gcos = q * dfac;
  *g = (float)(gcos * (double)rx);
  *h = (float)(gcos * cosine);
}
// dw of one weight from the two chains A = dot_i(g, x') and k = dot_i(h, 1)
FRMAP_TRACK_HD inline float frmap_head_fit_margin_dw(float A, float k, float rw, float w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float t1 = rw * A;
  if (!(rw < FRMAP_HEAD_FIT_MARGIN_RMAX)) return t1;
  const float r2 = rw * rw;
  const float t2 = r2 * k;
  const float t3 = t2 * w;
  return t1 - t3;
}

// the embedding step (the comment at the top, EMBED)
FRMAP_TRACK_HD inline bool frmap_head_fit_embed_shape_ok(int D, int E, int C) {
  return frmap_head_fit_shape_ok(D, E) && frmap_head_fit_shape_ok(E, C) && E <= FRMAP_HEAD_FIT_MAX_D;
}
FRMAP_TRACK_HD inline size_t frmap_head_fit_embed_state_size(int D, int E, int C, int amsgrad) {
  return frmap_head_fit_state_size(D, E, amsgrad) + frmap_head_fit_state_size(1, E, amsgrad) + frmap_head_fit_state_size(E, C, amsgrad);
}
FRMAP_TRACK_HD inline size_t frmap_head_fit_embed_workspace_size(int B, int E, int C) {
  return 4 * (5 * (size_t)B * (size_t)E + 5 * (size_t)E + 2 * (size_t)B + 2) + frmap_head_fit_margin_workspace_size(B, C);
}
struct FrmapHeadFitEmbedState {
  void *linear, *bn, *margin;            // the single layouts for (D, E), (1, E) and (E, C)
};
FRMAP_TRACK_HD inline FrmapHeadFitEmbedState frmap_head_fit_embed_state(void* state, int D, int E, int C, int amsgrad) {
  FrmapHeadFitEmbedState s;
  (void)C;
  s.linear = state;
  s.bn = (char*)state + frmap_head_fit_state_size(D, E, amsgrad);
  s.margin = (char*)s.bn + frmap_head_fit_state_size(1, E, amsgrad);
  return s;
}
struct FrmapHeadFitEmbedWork {
  float *a, *ah, *yp, *gy, *da, *mean32, *rstd, *uvar, *dbeta, *dgamma;
  int32_t *lab, *row_src1, *n1;
  void* margin;              // the margin workspace for (B, C)
};
FRMAP_TRACK_HD inline FrmapHeadFitEmbedWork frmap_head_fit_embed_work(void* workspace, int B, int E) {
  FrmapHeadFitEmbedWork k;
  const size_t be = (size_t)B * (size_t)E;
  k.a = (float*)workspace;
  k.ah = k.a + be;
  k.yp = k.ah + be;
  k.gy = k.yp + be;
  k.da = k.gy + be;
  k.mean32 = k.da + be;
  k.rstd = k.mean32 + E;
  k.uvar = k.rstd + E;
  k.dbeta = k.uvar + E;
  k.dgamma = k.dbeta + E;
  k.lab = (int32_t*)(k.dgamma + E);
  k.row_src1 = k.lab + B;
  k.n1 = k.row_src1 + B;
  k.margin = (void*)(k.n1 + 2);
  return k;
}
struct FrmapHeadFitBnHyper {
  float eps, momentum;
};
struct FrmapHeadFitBnStats {
  float mean32, rstd, uvar;
};
// the three statistics of a column from its float64 mean and its float64 sum of squared deviations over n1 >= 2 rows
FRMAP_TRACK_HD inline FrmapHeadFitBnStats frmap_head_fit_bn_stats(double mean, double sq, uint64_t n1, float eps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  FrmapHeadFitBnStats s;
  const double var = sq / (double)n1;
  const double ve = var + (double)eps;
  const double vn = var * (double)n1;
  s.mean32 = (float)mean;
  s.rstd = (float)(1.0 / sqrt(ve));
  s.uvar = (float)(vn / (double)(n1 - 1));
  return s;
}
FRMAP_TRACK_HD inline float frmap_head_fit_bn_ah(float a, float mean32, float rstd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = (double)a - (double)mean32;
  return (float)(d * (double)rstd);
}
// y' of one element: the affine map, then the dropout behind it (`kept` < 0: no mask)
FRMAP_TRACK_HD inline float frmap_head_fit_bn_y(float ah, float gamma, float beta, int kept, float keep_scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float t = gamma * ah;
  const float y = t + beta;
  return frmap_head_fit_xp(y, kept, keep_scale);
}
// gy of one element from the two chains S = dot_c(g rw, wc) and k = dot_c(h, 1)
FRMAP_TRACK_HD inline float frmap_head_fit_embed_gy(float S, float k, float rx, float yp, int kept, float keep_scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float gyp = S;
  if (rx < FRMAP_HEAD_FIT_MARGIN_RMAX) {
    const float r2 = rx * rx;
    const float t2 = r2 * k;
    const float t3 = t2 * yp;
    gyp = S - t3;
  }
  if (kept < 0) return gyp;
  return kept ? gyp * keep_scale : 0.0f;
}
FRMAP_TRACK_HD inline float frmap_head_fit_bn_da(float gy, float ah, float gamma, float rstd, float dbeta, float dgamma, uint64_t n1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double gs = (double)gamma * (double)rstd;
  const double mb = (double)dbeta / (double)n1;
  const double mg = (double)dgamma / (double)n1;
  const double u = (double)gy - mb;
  const double v = (double)ah * mg;
  const double t = u - v;
  return (float)(gs * t);
}
FRMAP_TRACK_HD inline float frmap_head_fit_bn_running(float r, float stat, float momentum) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float omm = 1.0f - momentum;
  const float p = omm * r;
  const float q = momentum * stat;
  return p + q;
}
