// The pair head-fitting step's host twin (csrc/head_fit_twin.h + head_fit_rule.h + tally_rule.h and the check programs' own
// head_fit_check_common.h, nothing else) as a stand-alone program, for a build with the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> tools/head_fit_pair_check.cpp -o check && ./check
// It sweeps the CPU shape table of tests/fit_pair_cases.py, (P, D, E), for three steps each with the learning rate changing per step,
// once with a mask and coupled decay and once without a mask, with decoupled decay and AMSGrad; with P >= 8 pairs 0 and 1 share their
// left row, pair 2 has left == right, and one pair each has a left index of -1, a NaN feature and a differ of 2.  Every buffer is a
// heap block of exactly its size, so the sanitizer sees any access outside them.  Checked on top of that:
//   * the two fills of the fresh workspace give the same bytes everywhere;
//   * an uncounted pair has row_src = -1 on both its rows, zero rows of ga and NaN in pair_loss and dist; a counted pair has a finite
//     loss and a distance in [1e-8, 2.001]; a row of a counted pair has ga orthogonal to its a (the normalisation's gradient);
//   * the header: t = 3, rows = 3 n, correct <= rows;
//   * the third step again with given_g on its own workspace gives the same weights and state;
//   * an all-declined batch changes nothing but the workspace and keeps t;
//   * refused calls write nothing.
// Exit status 0 and "self check passed" on success.
#define CHECK_SEED 24680u
#include "head_fit_check_common.h"

struct Problem {
  int N, P, D, E;
  Block<float> x, w, b;
  Block<int32_t> left, right, differ;
  Block<uint8_t> keep;
  Problem(int P_, int D_, int E_, bool dead)
      : N(P_ + 5), P(P_), D(D_), E(E_), x((size_t)N * D_), w((size_t)E_ * D_), b(E_), left(P_), right(P_), differ(P_), keep((size_t)2 * P_ * D_) {
    for (size_t i = 0; i < x.n; ++i) x.p[i] = small();
    for (int r = 0; r < N; ++r) x.p[(size_t)r * D] = 0.5f;                 // (no all-zero row)
    for (size_t i = 0; i < w.n; ++i) w.p[i] = small() * 0.25f;
    for (size_t i = 0; i < b.n; ++i) b.p[i] = small() * 0.05f;
    for (int p = 0; p < P; ++p) {
      left.p[p] = (int32_t)((p * 7 + 3) % N);
      right.p[p] = (int32_t)((p * 5 + 1) % N);
      differ.p[p] = (int32_t)(rnd() % 2);
    }
    for (size_t i = 0; i < keep.n; ++i) keep.p[i] = rnd() % 4 ? 1 : 0;
    for (int i = 0; i < 2 * P; ++i) keep.p[(size_t)i * D] = 1;
    if (P >= 8) {
      left.p[1] = left.p[0];
      right.p[2] = left.p[2];
      differ.p[2] = 1;
      left.p[4] = -1;
      differ.p[5] = 2;
      right.p[6] = N - 1;
      x.p[(size_t)(N - 1) * D + D / 2] = __builtin_nanf("");
    }
    if (dead)
      for (int p = 0; p < P; ++p) left.p[p] = p % 2 ? -1 : N;
  }
};

struct Run {
  Block<float> w, b;
  Block<uint8_t> state, work;
};

static const float LRS[3] = {1e-2f, 5e-3f, 2e-2f};
static const FrmapHeadFitPairHyper PH = {1.2f, 0.8f, 1.2f, 0.9f};

static const char* step(const Problem& p, Run& r, int variation, int s, bool clear, int given_g) {
  const int flags = (variation ? (FRMAP_HEAD_FIT_DECOUPLED | FRMAP_HEAD_FIT_AMSGRAD) : 0) | (clear ? FRMAP_HEAD_FIT_CLEAR : 0);
  const FrmapHeadFitHyper hy = {LRS[s % 3], 0.9f, 0.999f, 1e-8f, 1e-2f, 0.0f};
  return frmap_head_fit_pair_step_twin(p.x.p, p.left.p, p.right.p, p.differ.p, variation ? nullptr : p.keep.p, variation ? 1.0f : 1.0f / 0.75f,
                                       r.w.p, r.b.p, r.state.p, r.work.p, p.N, p.P, p.D, p.E, PH, hy, flags, given_g);
}

static Run steps(const Problem& p, int variation, int n_steps, int fill) {
  Run r = {p.w, p.b, Block<uint8_t>(frmap_head_fit_state_size(p.D, p.E, variation)), Block<uint8_t>(frmap_head_fit_pair_workspace_size(p.P, p.E), fill)};
  for (int s = 0; s < n_steps; ++s) {
    const char* why = step(p, r, variation, s, s == 0, 0);
    CHECK(!why, "pair twin refused: %s", why);
  }
  return r;
}

int main() {
  const int shapes[][3] = {{1, 1, 1}, {1, 3, 2}, {16, 64, 32}, {17, 65, 33}, {31, 128, 63}, {32, 129, 64}, {33, 512, 65}, {64, 512, 256}};
  long cases = 0;
  for (const auto& shape : shapes)
    for (int variation = 0; variation < 2; ++variation) {
      const int P = shape[0], D = shape[1], E = shape[2];
      const Problem p(P, D, E, false);
      const Run one = steps(p, variation, 3, 0xFF), two = steps(p, variation, 3, 0x5A);
      CHECK(one.w.same(two.w) && one.b.same(two.b) && one.state.same(two.state) && one.work.same(two.work), "P %d D %d E %d: the two fills differ", P, D, E);
      const uint64_t* head = (const uint64_t*)one.state.p;
      const uint64_t n = head[FRMAP_HEAD_FIT_N];
      CHECK(head[FRMAP_HEAD_FIT_T] == 3 && n >= 1 && head[FRMAP_HEAD_FIT_ROWS] == 3 * n && head[FRMAP_HEAD_FIT_CORRECT] <= 3 * n, "the header");
      const FrmapHeadFitPairWork wk = frmap_head_fit_pair_work(one.work.p, P, E);
      for (int q = 0; q < P; ++q) {
        const bool counted = wk.row_src[q] >= 0;
        CHECK(counted == (wk.row_src[P + q] >= 0), "pair %d is half counted", q);
        for (int side = 0; side < 2; ++side) {
          const float* a = wk.a + ((size_t)side * P + q) * E;
          const float* ga = wk.ga + ((size_t)side * P + q) * E;
          double dot = 0.0, na = 0.0, ng = 0.0;
          for (int e = 0; e < E; ++e) {
            if (!counted) CHECK(ga[e] == 0.0f, "ga of the uncounted pair %d", q);
            dot += (double)a[e] * ga[e];
            na += (double)a[e] * a[e];
            ng += (double)ga[e] * ga[e];
          }
          if (counted) CHECK(fabs(dot) <= 1e-5 * sqrt(na * ng) + 1e-30, "pair %d side %d: ga is not orthogonal to a (%g)", q, side, dot);
        }
        if (counted) CHECK(wk.pair_loss[q] >= 0.0f && wk.dist[q] >= 1e-8f && wk.dist[q] <= 2.001f, "pair %d: loss %g dist %g", q, wk.pair_loss[q], wk.dist[q]);
        else CHECK(wk.pair_loss[q] != wk.pair_loss[q] && wk.dist[q] != wk.dist[q], "pair %d is uncounted and its loss or distance is a number", q);
      }
      if (P >= 8) CHECK(wk.row_src[4] == -1 && wk.row_src[P + 5] == -1 && wk.row_src[6] == -1 && wk.row_src[0] >= 0 && wk.row_src[2] == wk.row_src[P + 2], "the bad pairs");
      {   // the third step again with given_g on its own workspace
        Run base = steps(p, variation, 2, 0);
        Run again = {base.w, base.b, base.state, one.work};
        CHECK(!step(p, again, variation, 2, false, 1), "given_g refused");
        CHECK(again.w.same(one.w) && again.b.same(one.b) && again.state.same(one.state) && again.work.same(one.work), "the third step with given_g");
      }
      {   // every pair declined: nothing but the workspace changes, t stays
        const Problem dead(P, D, E, true);
        const Run r = steps(dead, variation, 1, 0xFF);
        CHECK(r.w.same(dead.w) && r.b.same(dead.b), "an all-declined batch moved a weight");
        for (size_t i = 0; i < r.state.n; ++i) CHECK(r.state.p[i] == 0, "an all-declined batch wrote state byte %zu", i);
      }
      ++cases;
    }
  {   // refusals: nothing is written
    const Problem p(4, 3, 5, false);
    Run r = {p.w, p.b, Block<uint8_t>(frmap_head_fit_state_size(3, 5, 0)), Block<uint8_t>(frmap_head_fit_pair_workspace_size(4, 5))};
    const FrmapHeadFitHyper hy = {1e-2f, 0.9f, 0.999f, 1e-8f, 0.0f, 0.0f};
#define REFUSED(word, N_, P_, D_, E_, flags_, w_)                                                                                               \
  do {                                                                                                                                          \
    const char* why = frmap_head_fit_pair_step_twin(p.x.p, p.left.p, p.right.p, p.differ.p, nullptr, 1.0f, w_, r.b.p, r.state.p, r.work.p, N_,   \
                                                    P_, D_, E_, PH, hy, flags_, 0);                                                            \
    CHECK(why && strstr(why, word), "accepted, or %s is not named: %s", word, why ? why : "(accepted)");                                        \
  } while (0)
    REFUSED("N", 0, 4, 3, 5, 0, r.w.p);
    REFUSED("P", p.N, 0, 3, 5, 0, r.w.p);
    REFUSED("P", p.N, FRMAP_HEAD_FIT_MAX_P + 1, 3, 5, 0, r.w.p);
    REFUSED("D", p.N, 4, 65537, 5, 0, r.w.p);
    REFUSED("E", p.N, 4, 3, 0, 0, r.w.p);
    REFUSED("flags", p.N, 4, 3, 5, 8, r.w.p);
    REFUSED("null pointer", p.N, 4, 3, 5, 0, (float*)nullptr);
    CHECK(r.w.same(p.w) && r.b.same(p.b), "a refused call wrote the weights");
    for (size_t i = 0; i < r.state.n; ++i) CHECK(r.state.p[i] == 0, "a refused call wrote the state");
    for (size_t i = 0; i < r.work.n; ++i) CHECK(r.work.p[i] == 0, "a refused call wrote the workspace");
  }
  CHECK(frmap_head_fit_pair_workspace_size(32, 256) == 4 * (4 * 32 * 256 + 4 * 32) && frmap_head_fit_pair_shape_ok(FRMAP_HEAD_FIT_MAX_P, 1, 1) &&
            !frmap_head_fit_pair_shape_ok(FRMAP_HEAD_FIT_MAX_P + 1, 1, 1),
        "sizes");
  printf("%ld cases\nself check passed\n", cases);
  return 0;
}
