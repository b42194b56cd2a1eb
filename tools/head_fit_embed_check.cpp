// The embedding head-fitting step's host twin (csrc/head_fit_twin.h + head_fit_rule.h + tally_rule.h and the check programs' own
// head_fit_check_common.h, nothing else) as a stand-alone program, for a build with the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> tools/head_fit_embed_check.cpp -o check && ./check
// It sweeps a part of the shape table of tests/fit_embed_cases.py, (B, D, E, C), for three steps each with the learning rate, the scale,
// the margin, the easy margin and the smoothing changing per step, once with a mask and coupled decay and once without a mask, with
// decoupled decay and AMSGrad; with B >= 8 one row each has an index of -1, a label of C and a NaN feature.  Every buffer is a heap block
// of exactly its size, so the sanitizer sees any access outside them.  Checked on top of that:
//   * the two fills of the fresh workspace give the same bytes everywhere;
//   * a declined row has row_src1 = -1, lab = -1 and zero rows of a, ah, y', gy and da; n1 is the count of the others;
//   * the three headers: t = 3 and n = n1 in each, rows = 3 n1 and correct <= rows in the margin state, zero figures in the other two;
//   * the third step again with given = 7 on its own workspace gives the same parameters and state;
//   * a batch with one counted row, and a NaN in gamma, change nothing but the workspace: every byte of the parameters and the state;
//   * refused calls write nothing.
// Exit status 0 and "self check passed" on success.
#define CHECK_SEED 24680u
#include "head_fit_check_common.h"

struct Problem {
  int N, B, D, E, C;
  Block<float> x, w1, gamma, beta, rm, rv, wc;
  Block<int32_t> labels, rows;
  Block<uint8_t> keep;
  Problem(int B_, int D_, int E_, int C_, int alive)
      : N(B_ + 3), B(B_), D(D_), E(E_), C(C_), x((size_t)N * D_), w1((size_t)E_ * D_), gamma(E_), beta(E_), rm(E_), rv(E_), wc((size_t)C_ * E_),
        labels(N), rows(B_), keep((size_t)B_ * E_) {
    for (size_t i = 0; i < x.n; ++i) x.p[i] = small();
    for (size_t i = 0; i < w1.n; ++i) w1.p[i] = small() * 0.5f;
    for (int j = 0; j < E; ++j) {
      w1.p[(size_t)j * D] = 0.25f + 0.125f * (float)(j % 3);
      gamma.p[j] = 1.0f + 0.125f * small();
      beta.p[j] = 0.125f * small();
      rm.p[j] = 0.125f * small();
      rv.p[j] = 1.0f + 0.0625f * (float)(j % 5);
    }
    for (size_t i = 0; i < wc.n; ++i) wc.p[i] = small() * 0.5f;
    for (int c = 0; c < C; ++c) wc.p[(size_t)c * E] = 0.25f;
    for (int r = 0; r < N; ++r) labels.p[r] = (int32_t)(rnd() % (uint32_t)C);
    for (int i = 0; i < B; ++i) rows.p[i] = (int32_t)((i * 7 + 2) % N);
    for (size_t i = 0; i < keep.n; ++i) keep.p[i] = rnd() % 2 ? 1 : 0;
    for (int i = 0; i < B; ++i) keep.p[(size_t)i * E] = 1;
    if (B >= 8) {
      rows.p[1] = -1;
      rows.p[2] = N - 1;
      labels.p[N - 1] = C;
      rows.p[3] = N - 2;
      x.p[(size_t)(N - 2) * D + D / 2] = __builtin_nanf("");
    }
    if (alive >= 0)
      for (int i = alive; i < B; ++i) rows.p[i] = i % 2 ? -1 : N;       // only the first `alive` rows are counted
  }
};

struct Run {
  Block<float> w1, gamma, beta, rm, rv, wc;
  Block<uint8_t> state, work;
  bool same_params(const Run& o) const {
    return w1.same(o.w1) && gamma.same(o.gamma) && beta.same(o.beta) && rm.same(o.rm) && rv.same(o.rv) && wc.same(o.wc) && state.same(o.state);
  }
};

static const float LRS[3] = {1e-2f, 5e-3f, 2e-2f}, SCALES[3] = {7.2f, 9.6f, 5.28f}, MARGINS[3] = {0.0f, 0.27f, 0.45f};

static const char* step(const Problem& p, Run& r, int variation, int s, bool clear, int given) {
  const int flags = (variation ? (FRMAP_HEAD_FIT_DECOUPLED | FRMAP_HEAD_FIT_AMSGRAD) : 0) | (clear ? FRMAP_HEAD_FIT_CLEAR : 0) |
                    ((s & 1) ? FRMAP_HEAD_FIT_EASY_MARGIN : 0);
  const FrmapHeadFitHyper hy = {LRS[s % 3], 0.9f, 0.999f, 1e-8f, 1e-2f, s ? 0.05f : 0.0f};
  const FrmapHeadFitMarginHyper mh = {SCALES[s % 3], MARGINS[s % 3]};
  const FrmapHeadFitBnHyper bh = {1e-5f, 0.1f};
  return frmap_head_fit_embed_step_twin(p.x.p, p.labels.p, p.rows.p, variation ? nullptr : p.keep.p, variation ? 1.0f : 2.0f, r.w1.p, r.gamma.p,
                                        r.beta.p, r.rm.p, r.rv.p, r.wc.p, r.state.p, r.work.p, p.N, p.B, p.D, p.E, p.C, bh, mh, hy, flags, given);
}

static Run fresh(const Problem& p, int variation, int fill) {
  return Run{p.w1, p.gamma, p.beta, p.rm, p.rv, p.wc, Block<uint8_t>(frmap_head_fit_embed_state_size(p.D, p.E, p.C, variation)),
             Block<uint8_t>(frmap_head_fit_embed_workspace_size(p.B, p.E, p.C), fill)};
}

static Run steps(const Problem& p, int variation, int n_steps, int fill) {
  Run r = fresh(p, variation, fill);
  for (int s = 0; s < n_steps; ++s) {
    const char* why = step(p, r, variation, s, s == 0, 0);
    CHECK(!why, "embed twin refused: %s", why);
  }
  return r;
}

int main() {
  const int shapes[][4] = {{3, 3, 3, 3}, {2, 31, 33, 2}, {31, 32, 31, 32}, {33, 31, 1, 33}, {33, 3, 33, 1}, {129, 3, 3, 3}, {3, 129, 3, 2}, {2, 3, 129, 3}};
  long cases = 0;
  for (const auto& shape : shapes)
    for (int variation = 0; variation < 2; ++variation) {
      const int B = shape[0], D = shape[1], E = shape[2], C = shape[3];
      const Problem p(B, D, E, C, -1);
      const Run one = steps(p, variation, 3, 0xFF), two = steps(p, variation, 3, 0x5A);
      CHECK(one.same_params(two) && one.work.same(two.work), "B %d D %d E %d C %d: the two fills differ", B, D, E, C);
      const FrmapHeadFitEmbedState es = frmap_head_fit_embed_state(one.state.p, D, E, C, variation);
      const FrmapHeadFitEmbedWork wk = frmap_head_fit_embed_work(one.work.p, B, E);
      const uint64_t n1 = (uint64_t)wk.n1[0];
      const uint64_t *h1 = (const uint64_t*)es.linear, *h2 = (const uint64_t*)es.bn, *h3 = (const uint64_t*)es.margin;
      CHECK(n1 >= 2 && h1[FRMAP_HEAD_FIT_T] == 3 && h2[FRMAP_HEAD_FIT_T] == 3 && h3[FRMAP_HEAD_FIT_T] == 3, "t of the three headers");
      CHECK(h1[FRMAP_HEAD_FIT_N] == n1 && h2[FRMAP_HEAD_FIT_N] == n1 && h3[FRMAP_HEAD_FIT_N] == n1, "n of the three headers");
      CHECK(h3[FRMAP_HEAD_FIT_ROWS] == 3 * n1 && h3[FRMAP_HEAD_FIT_CORRECT] <= 3 * n1, "the figures");
      for (int k = FRMAP_HEAD_FIT_ROWS; k <= FRMAP_HEAD_FIT_LOSS_Q; ++k) CHECK(h1[k] == 0 && h2[k] == 0, "a figure word of header 1 or 2");
      uint64_t counted = 0;
      for (int i = 0; i < B; ++i) {
        const bool ok = wk.row_src1[i] >= 0;
        counted += ok ? 1 : 0;
        CHECK(ok == (wk.lab[i] >= 0), "row %d: lab and row_src1 disagree", i);
        for (int j = 0; j < E; ++j) {
          const size_t at = (size_t)i * E + j;
          if (!ok) CHECK(wk.a[at] == 0.0f && wk.ah[at] == 0.0f && wk.yp[at] == 0.0f && wk.gy[at] == 0.0f && wk.da[at] == 0.0f, "row %d is declined and not zero", i);
          else CHECK(wk.ah[at] == wk.ah[at] && wk.da[at] == wk.da[at], "row %d unit %d is NaN", i, j);
        }
      }
      CHECK(counted == n1, "n1");
      if (B >= 8) CHECK(wk.row_src1[1] == -1 && wk.row_src1[2] == -1 && wk.row_src1[3] == -1 && wk.row_src1[0] >= 0, "the bad rows");
      {   // the third step again with every float64 stage given, on its own workspace
        Run base = steps(p, variation, 2, 0);
        Run again = {base.w1, base.gamma, base.beta, base.rm, base.rv, base.wc, base.state, one.work};
        CHECK(!step(p, again, variation, 2, false, 7), "given = 7 refused");
        CHECK(again.same_params(one) && again.work.same(one.work), "the third step with given = 7");
      }
      {   // one counted row: the step is not taken
        const Problem lone(B, D, E, C, 1);
        const Run r = steps(lone, variation, 1, 0xFF), untouched = fresh(lone, variation, 0);
        CHECK(r.same_params(untouched), "a batch with one counted row moved a parameter or the state");
      }
      {   // a NaN in gamma poisons a column of y': the margin stage declines every row, n2 != n1
        Problem bad(B, D, E, C, -1);
        bad.gamma.p[E / 2] = __builtin_nanf("");
        for (int i = 0; i < B; ++i) bad.keep.p[(size_t)i * E + E / 2] = 1;     // (the poisoned column is kept in every row)
        const Run r = steps(bad, variation, 1, 0xFF), untouched = fresh(bad, variation, 0);
        CHECK(r.same_params(untouched), "a NaN in gamma moved a parameter or the state");
      }
      ++cases;
    }
  {   // refusals: nothing is written
    const Problem p(4, 3, 2, 5, -1);
    Run r = fresh(p, 0, 0);
    const Run untouched = fresh(p, 0, 0);
    const FrmapHeadFitHyper hy = {1e-2f, 0.9f, 0.999f, 1e-8f, 0.0f, 0.0f};
    const FrmapHeadFitMarginHyper mh = {9.6f, 0.45f};
    const FrmapHeadFitBnHyper bh = {1e-5f, 0.1f};
#define REFUSED(word, N_, B_, D_, E_, C_, flags_, w_, given_)                                                                                  \
  do {                                                                                                                                         \
    const char* why = frmap_head_fit_embed_step_twin(p.x.p, p.labels.p, p.rows.p, nullptr, 1.0f, w_, r.gamma.p, r.beta.p, r.rm.p, r.rv.p,       \
                                                     r.wc.p, r.state.p, r.work.p, N_, B_, D_, E_, C_, bh, mh, hy, flags_, given_);             \
    CHECK(why && strstr(why, word), "accepted, or %s is not named: %s", word, why ? why : "(accepted)");                                       \
  } while (0)
    REFUSED("N", 0, 4, 3, 2, 5, 0, r.w1.p, 0);
    REFUSED("B", p.N, 0, 3, 2, 5, 0, r.w1.p, 0);
    REFUSED("B", p.N, FRMAP_HEAD_FIT_MAX_B + 1, 3, 2, 5, 0, r.w1.p, 0);
    REFUSED("D", p.N, 4, 65537, 2, 5, 0, r.w1.p, 0);
    REFUSED("E", p.N, 4, 3, 0, 5, 0, r.w1.p, 0);
    REFUSED("E", p.N, 4, 3, 65537, 5, 0, r.w1.p, 0);
    REFUSED("C", p.N, 4, 3, 2, 0, 0, r.w1.p, 0);
    REFUSED("flags", p.N, 4, 3, 2, 5, 8, r.w1.p, 0);
    REFUSED("flags", p.N, 4, 3, 2, 5, 32, r.w1.p, 0);
    REFUSED("null pointer", p.N, 4, 3, 2, 5, 0, (float*)nullptr, 0);
    REFUSED("given", p.N, 4, 3, 2, 5, 0, r.w1.p, 8);
    CHECK(r.same_params(untouched) && r.work.same(untouched.work), "a refused call wrote something");
  }
  CHECK(frmap_head_fit_embed_workspace_size(32, 16, 256) == 4 * (5 * 32 * 16 + 5 * 16 + 2 * 32 + 2) + frmap_head_fit_margin_workspace_size(32, 256), "sizes");
  CHECK(frmap_head_fit_embed_state_size(8, 16, 5, 1) % 8 == 0 && frmap_head_fit_state_size(1, 16, 1) % 8 == 0, "state parts");
  printf("%ld cases\nself check passed\n", cases);
  return 0;
}
