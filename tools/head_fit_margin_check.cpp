// The margin head-fitting step's host twin (csrc/head_fit_twin.h + head_fit_rule.h + tally_rule.h and the check programs' own
// head_fit_check_common.h, nothing else) as a stand-alone program, for a build with the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> tools/head_fit_margin_check.cpp -o check && ./check
// It sweeps the diagonal and the corners of the shape table of tests/fit_margin_cases.py, (B, D, C), for three steps each with the
// learning rate, the scale, the margin, the easy margin and the smoothing changing per step, once with a mask and coupled decay and
// once without a mask, with decoupled decay and AMSGrad; with B >= 8 one row each has an index of -1, a label of C and a NaN feature,
// one row is zeros and one class centre is zeros.  Every buffer is a heap block of exactly its size, so the sanitizer sees any access
// outside them.  Checked on top of that:
//   * the two fills of the fresh workspace give the same bytes everywhere;
//   * a declined row has row_src = -1, rx = +0, zero rows of z, cosv, g and h and a NaN loss; a counted row has a finite loss, rx > 0 and
//     |cosv| at most the clamp bound; every rw is positive;
//   * the header: t = 3, rows = 3 n, correct <= rows;
//   * the third step again with given_g on its own workspace gives the same weights and state;
//   * an all-declined batch changes nothing but the workspace and keeps t;
//   * refused calls write nothing.
// Exit status 0 and "self check passed" on success.
#define CHECK_SEED 13579u
#include "head_fit_check_common.h"

struct Problem {
  int N, B, D, C;
  Block<float> x, w;
  Block<int32_t> labels, rows;
  Block<uint8_t> keep;
  Problem(int B_, int D_, int C_, bool dead) : N(B_ + 3), B(B_), D(D_), C(C_), x((size_t)N * D_), w((size_t)C_ * D_), labels(N), rows(B_), keep((size_t)B_ * D_) {
    for (size_t i = 0; i < x.n; ++i) x.p[i] = small();
    for (int r = 0; r < N; ++r) x.p[(size_t)r * D] = 0.5f;                 // (no all-zero row by chance)
    for (size_t i = 0; i < w.n; ++i) w.p[i] = small() * 0.5f;
    for (int c = 0; c < C; ++c) w.p[(size_t)c * D] = 0.25f;
    for (int r = 0; r < N; ++r) labels.p[r] = (int32_t)(rnd() % (uint32_t)C);
    for (int i = 0; i < B; ++i) rows.p[i] = (int32_t)((i * 7 + 2) % N);
    for (size_t i = 0; i < keep.n; ++i) keep.p[i] = rnd() % 2 ? 1 : 0;
    for (int i = 0; i < B; ++i) keep.p[(size_t)i * D] = 1;
    if (B >= 8) {
      rows.p[1] = -1;
      rows.p[2] = N - 1;
      labels.p[N - 1] = C;
      rows.p[3] = N - 2;
      x.p[(size_t)(N - 2) * D + D / 2] = __builtin_nanf("");
      for (int k = 0; k < D; ++k) x.p[(size_t)rows.p[4] * D + k] = 0.0f;
      if (C >= 2)
        for (int k = 0; k < D; ++k) w.p[(size_t)(C - 1) * D + k] = 0.0f;
    }
    if (dead)
      for (int i = 0; i < B; ++i) rows.p[i] = i % 2 ? -1 : N;
  }
};

struct Run {
  Block<float> w;
  Block<uint8_t> state, work;
};

static const float LRS[3] = {1e-2f, 5e-3f, 2e-2f}, SCALES[3] = {7.2f, 9.6f, 5.28f}, MARGINS[3] = {0.0f, 0.27f, 0.45f};

static const char* step(const Problem& p, Run& r, int variation, int s, bool clear, int given_g) {
  const int flags = (variation ? (FRMAP_HEAD_FIT_DECOUPLED | FRMAP_HEAD_FIT_AMSGRAD) : 0) | (clear ? FRMAP_HEAD_FIT_CLEAR : 0) |
                    ((s & 1) ? FRMAP_HEAD_FIT_EASY_MARGIN : 0);
  const FrmapHeadFitHyper hy = {LRS[s % 3], 0.9f, 0.999f, 1e-8f, 1e-2f, s ? 0.05f : 0.0f};
  const FrmapHeadFitMarginHyper mh = {SCALES[s % 3], MARGINS[s % 3]};
  return frmap_head_fit_margin_step_twin(p.x.p, p.labels.p, p.rows.p, variation ? nullptr : p.keep.p, variation ? 1.0f : 2.0f, r.w.p, r.state.p,
                                         r.work.p, p.N, p.B, p.D, p.C, mh, hy, flags, given_g);
}

static Run steps(const Problem& p, int variation, int n_steps, int fill) {
  Run r = {p.w, Block<uint8_t>(frmap_head_fit_state_size(p.D, p.C, variation)), Block<uint8_t>(frmap_head_fit_margin_workspace_size(p.B, p.C), fill)};
  for (int s = 0; s < n_steps; ++s) {
    const char* why = step(p, r, variation, s, s == 0, 0);
    CHECK(!why, "margin twin refused: %s", why);
  }
  return r;
}

int main() {
  const int shapes[][3] = {{1, 1, 1}, {31, 3, 2}, {32, 64, 18}, {33, 65, 33}, {65, 512, 65}, {1, 512, 65}, {65, 1, 1}, {65, 3, 65}};
  long cases = 0;
  for (const auto& shape : shapes)
    for (int variation = 0; variation < 2; ++variation) {
      const int B = shape[0], D = shape[1], C = shape[2];
      const Problem p(B, D, C, false);
      const Run one = steps(p, variation, 3, 0xFF), two = steps(p, variation, 3, 0x5A);
      CHECK(one.w.same(two.w) && one.state.same(two.state) && one.work.same(two.work), "B %d D %d C %d: the two fills differ", B, D, C);
      const uint64_t* head = (const uint64_t*)one.state.p;
      const uint64_t n = head[FRMAP_HEAD_FIT_N];
      CHECK(head[FRMAP_HEAD_FIT_T] == 3 && n >= 1 && head[FRMAP_HEAD_FIT_ROWS] == 3 * n && head[FRMAP_HEAD_FIT_CORRECT] <= 3 * n, "the header");
      const FrmapHeadFitMarginWork wk = frmap_head_fit_margin_work(one.work.p, B, C);
      for (int c = 0; c < C; ++c) CHECK(wk.rw[c] > 0.0f && wk.rw[c] <= FRMAP_HEAD_FIT_MARGIN_RMAX, "rw of class %d: %g", c, wk.rw[c]);
      for (int i = 0; i < B; ++i) {
        const bool counted = wk.row_src[i] >= 0;
        for (int c = 0; c < C; ++c) {
          const size_t at = (size_t)i * C + c;
          if (!counted) CHECK(wk.z[at] == 0.0f && wk.cosv[at] == 0.0f && wk.g[at] == 0.0f && wk.h[at] == 0.0f, "row %d is declined and not zero", i);
          else CHECK(fabsf(wk.cosv[at]) <= FRMAP_HEAD_FIT_MARGIN_HI && wk.g[at] == wk.g[at] && wk.h[at] == wk.h[at], "row %d class %d: cosv %g", i, c, wk.cosv[at]);
        }
        if (counted) CHECK(wk.row_loss[i] >= 0.0f && wk.rx[i] > 0.0f, "row %d: loss %g rx %g", i, wk.row_loss[i], wk.rx[i]);
        else CHECK(wk.row_loss[i] != wk.row_loss[i] && wk.rx[i] == 0.0f, "row %d is declined and its loss or rx is a number", i);
      }
      if (B >= 8) CHECK(wk.row_src[1] == -1 && wk.row_src[2] == -1 && wk.row_src[3] == -1 && wk.row_src[0] >= 0 && wk.rx[4] == FRMAP_HEAD_FIT_MARGIN_RMAX, "the bad rows");
      {   // the third step again with given_g on its own workspace
        Run base = steps(p, variation, 2, 0);
        Run again = {base.w, base.state, one.work};
        CHECK(!step(p, again, variation, 2, false, 1), "given_g refused");
        CHECK(again.w.same(one.w) && again.state.same(one.state) && again.work.same(one.work), "the third step with given_g");
      }
      {   // every row declined: nothing but the workspace changes, t stays
        const Problem dead(B, D, C, true);
        const Run r = steps(dead, variation, 1, 0xFF);
        CHECK(r.w.same(dead.w), "an all-declined batch moved a weight");
        for (size_t i = 0; i < r.state.n; ++i) CHECK(r.state.p[i] == 0, "an all-declined batch wrote state byte %zu", i);
      }
      ++cases;
    }
  {   // refusals: nothing is written
    const Problem p(4, 3, 5, false);
    Run r = {p.w, Block<uint8_t>(frmap_head_fit_state_size(3, 5, 0)), Block<uint8_t>(frmap_head_fit_margin_workspace_size(4, 5))};
    const FrmapHeadFitHyper hy = {1e-2f, 0.9f, 0.999f, 1e-8f, 0.0f, 0.0f};
    const FrmapHeadFitMarginHyper mh = {9.6f, 0.45f};
#define REFUSED(word, N_, B_, D_, C_, flags_, w_)                                                                                              \
  do {                                                                                                                                         \
    const char* why = frmap_head_fit_margin_step_twin(p.x.p, p.labels.p, p.rows.p, nullptr, 1.0f, w_, r.state.p, r.work.p, N_, B_, D_, C_, mh,  \
                                                      hy, flags_, 0);                                                                          \
    CHECK(why && strstr(why, word), "accepted, or %s is not named: %s", word, why ? why : "(accepted)");                                       \
  } while (0)
    REFUSED("N", 0, 4, 3, 5, 0, r.w.p);
    REFUSED("B", p.N, 0, 3, 5, 0, r.w.p);
    REFUSED("B", p.N, FRMAP_HEAD_FIT_MAX_B + 1, 3, 5, 0, r.w.p);
    REFUSED("D", p.N, 4, 65537, 5, 0, r.w.p);
    REFUSED("C", p.N, 4, 3, 0, 0, r.w.p);
    REFUSED("flags", p.N, 4, 3, 5, 8, r.w.p);
    REFUSED("flags", p.N, 4, 3, 5, 32, r.w.p);
    REFUSED("null pointer", p.N, 4, 3, 5, 0, (float*)nullptr);
    CHECK(r.w.same(p.w), "a refused call wrote the weights");
    for (size_t i = 0; i < r.state.n; ++i) CHECK(r.state.p[i] == 0, "a refused call wrote the state");
    for (size_t i = 0; i < r.work.n; ++i) CHECK(r.work.p[i] == 0, "a refused call wrote the workspace");
  }
  CHECK(frmap_head_fit_margin_workspace_size(32, 256) == 4 * (4 * 32 * 256 + 3 * 32 + 256), "sizes");
  printf("%ld cases\nself check passed\n", cases);
  return 0;
}
