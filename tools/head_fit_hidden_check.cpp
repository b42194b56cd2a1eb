// The hidden-layer head-fitting step's host twin (csrc/head_fit_twin.h + head_fit_rule.h + tally_rule.h and the check programs' own
// head_fit_check_common.h, nothing else) as a stand-alone program, for a build with the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> tools/head_fit_hidden_check.cpp -o check && ./check
// It sweeps the CPU shape table of tests/fit_hidden_cases.py, (B, D, Hd, C), for three steps each with the learning rate changing
// per step, once with both masks and coupled decay and once with keep2 only, decoupled decay, AMSGrad and label smoothing; with
// B >= 4 one batch row has rows = -1, one a label of C and one a NaN feature.  Every buffer is a heap block of exactly its size, so
// the sanitizer sees any access outside them.  Checked on top of that:
//   * the two fills of the fresh workspace give the same bytes everywhere;
//   * layer 2 of the step holds the bytes of the single twin run on (h, lab, keep2) alone: w2, b2, the second part of the state and
//     the tail of the workspace;
//   * the first part's t and n are the second's and its figure words stay 0;
//   * a declined row has lab = -1 and a zero row of h and da; da is zero wherever h is not positive or the unit is masked;
//   * an all-declined batch changes nothing but the workspace and keeps t;
//   * refused calls write nothing.
// Exit status 0 and "self check passed" on success.
#define CHECK_SEED 97531u
#include "head_fit_check_common.h"

struct Problem {
  int N, B, D, Hd, C;
  Block<float> x, w1, b1, w2, b2;
  Block<int32_t> labels, rows;
  Block<uint8_t> keep1, keep2;
  Problem(int B_, int D_, int Hd_, int C_, bool dead)
      : N(B_ + 5), B(B_), D(D_), Hd(Hd_), C(C_), x((size_t)N * D_), w1((size_t)Hd_ * D_), b1(Hd_), w2((size_t)C_ * Hd_), b2(C_), labels(N), rows(B_),
        keep1((size_t)B_ * D_), keep2((size_t)B_ * Hd_) {
    for (size_t i = 0; i < x.n; ++i) x.p[i] = small();
    for (size_t i = 0; i < w1.n; ++i) w1.p[i] = small() * 0.25f;
    for (size_t i = 0; i < b1.n; ++i) b1.p[i] = small() * 0.05f;
    for (size_t i = 0; i < w2.n; ++i) w2.p[i] = small() * 0.25f;
    for (size_t i = 0; i < b2.n; ++i) b2.p[i] = small() * 0.05f;
    for (int i = 0; i < N; ++i) labels.p[i] = (int32_t)(rnd() % (uint32_t)C);
    for (int i = 0; i < B; ++i) rows.p[i] = (int32_t)((i * 7 + 3) % N);
    for (size_t i = 0; i < keep1.n; ++i) keep1.p[i] = rnd() % 4 ? 1 : 0;
    for (size_t i = 0; i < keep2.n; ++i) keep2.p[i] = rnd() % 2 ? 1 : 0;
    if (B >= 4) {
      rows.p[1] = -1;
      labels.p[rows.p[2]] = C;
      x.p[(size_t)rows.p[3] * D + D / 2] = __builtin_nanf("");
    }
    if (dead)
      for (int i = 0; i < B; ++i) rows.p[i] = i % 2 ? -1 : N;
  }
};

struct Run {
  Block<float> w1, b1, w2, b2;
  Block<uint8_t> state, work;
};

static const float LRS[3] = {1e-2f, 5e-3f, 2e-2f};

static Run steps(const Problem& p, int variation, int n_steps, int fill) {
  const int flags = variation ? (FRMAP_HEAD_FIT_DECOUPLED | FRMAP_HEAD_FIT_AMSGRAD) : 0;
  Run r = {p.w1, p.b1, p.w2, p.b2, Block<uint8_t>(frmap_head_fit_hidden_state_size(p.D, p.Hd, p.C, flags & FRMAP_HEAD_FIT_AMSGRAD)),
           Block<uint8_t>(frmap_head_fit_hidden_workspace_size(p.B, p.Hd, p.C), fill)};
  for (int s = 0; s < n_steps; ++s) {
    const FrmapHeadFitHyper hy = {LRS[s % 3], 0.9f, 0.999f, 1e-8f, 1e-2f, variation ? 0.1f : 0.0f};
    const char* why = frmap_head_fit_hidden_step_twin(p.x.p, p.labels.p, p.rows.p, variation ? nullptr : p.keep1.p, variation ? 1.0f : 1.0f / 0.75f,
                                                      p.keep2.p, 2.0f, r.w1.p, r.b1.p, r.w2.p, r.b2.p, r.state.p, r.work.p, p.N, p.B, p.D, p.Hd, p.C,
                                                      hy, flags | (s == 0 ? FRMAP_HEAD_FIT_CLEAR : 0), 0);
    CHECK(!why, "hidden twin refused: %s", why);
  }
  return r;
}

int main() {
  const int shapes[][4] = {{1, 1, 1, 1}, {5, 2, 3, 1}, {31, 3, 33, 2}, {32, 64, 32, 18}, {33, 65, 65, 33}, {65, 129, 129, 129}};
  long cases = 0;
  for (const auto& shape : shapes)
    for (int variation = 0; variation < 2; ++variation) {
      const int B = shape[0], D = shape[1], Hd = shape[2], C = shape[3];
      const int flags = variation ? (FRMAP_HEAD_FIT_DECOUPLED | FRMAP_HEAD_FIT_AMSGRAD) : 0, ams = flags & FRMAP_HEAD_FIT_AMSGRAD;
      const Problem p(B, D, Hd, C, false);
      const Run one = steps(p, variation, 3, 0xFF), two = steps(p, variation, 3, 0x5A);
      CHECK(one.w1.same(two.w1) && one.b1.same(two.b1) && one.w2.same(two.w2) && one.b2.same(two.b2) && one.state.same(two.state) &&
                one.work.same(two.work),
            "B %d D %d Hd %d C %d: the two fills differ", B, D, Hd, C);
      const size_t n1 = frmap_head_fit_state_size(D, Hd, ams), n2 = frmap_head_fit_state_size(Hd, C, ams);
      CHECK(n1 % 8 == 0 && n2 % 8 == 0 && one.state.n == n1 + n2, "state sizes %zu + %zu", n1, n2);
      const uint64_t *h1 = (const uint64_t*)one.state.p, *h2 = (const uint64_t*)(one.state.p + n1);
      CHECK(h1[FRMAP_HEAD_FIT_T] == h2[FRMAP_HEAD_FIT_T] && h1[FRMAP_HEAD_FIT_N] == h2[FRMAP_HEAD_FIT_N], "t and n of layer 1 are not layer 2's");
      CHECK(h1[2] == 0 && h1[3] == 0 && h1[4] == 0 && h1[5] == 0 && h1[6] == 0 && h1[7] == 0, "figure words of layer 1 written");
      CHECK(h2[FRMAP_HEAD_FIT_T] == 3 && h2[FRMAP_HEAD_FIT_N] >= 1 && h2[FRMAP_HEAD_FIT_ROWS] == 3 * h2[FRMAP_HEAD_FIT_N], "header of layer 2");
      {   // the last step again, by hand: layer 2 is the single twin on (h, lab, keep2)
        Run base = steps(p, variation, 2, 0);
        Run full = {base.w1, base.b1, base.w2, base.b2, base.state, Block<uint8_t>(base.work.n, 0xFF)};
        const FrmapHeadFitHyper hy = {LRS[2], 0.9f, 0.999f, 1e-8f, 1e-2f, variation ? 0.1f : 0.0f};
        CHECK(!frmap_head_fit_hidden_step_twin(p.x.p, p.labels.p, p.rows.p, variation ? nullptr : p.keep1.p, variation ? 1.0f : 1.0f / 0.75f,
                                               p.keep2.p, 2.0f, full.w1.p, full.b1.p, full.w2.p, full.b2.p, full.state.p, full.work.p, p.N, B, D, Hd, C,
                                               hy, flags, 0),
              "third step refused");
        CHECK(full.w1.same(one.w1) && full.w2.same(one.w2) && full.state.same(one.state) && full.work.same(one.work), "the third step by hand");
        const FrmapHeadFitHiddenWork wk = frmap_head_fit_hidden_work(full.work.p, B, Hd);
        Block<float> h((size_t)B * Hd), w2(base.w2), b2(base.b2);
        Block<int32_t> lab(B);
        memcpy(h.p, wk.h, h.n * 4);
        memcpy(lab.p, wk.lab, (size_t)B * 4);
        Block<uint8_t> st2(n2), wk2(frmap_head_fit_workspace_size(B, C), 0x5A);
        memcpy(st2.p, base.state.p + n1, n2);
        CHECK(!frmap_head_fit_step_twin(h.p, lab.p, nullptr, p.keep2.p, 2.0f, w2.p, b2.p, st2.p, wk2.p, B, B, Hd, C, hy, flags, 0), "single twin refused");
        CHECK(w2.same(full.w2) && b2.same(full.b2) && memcmp(st2.p, full.state.p + n1, n2) == 0 && memcmp(wk2.p, wk.layer2, wk2.n) == 0,
              "B %d D %d Hd %d C %d: layer 2 differs from the single twin on (h, lab, keep2)", B, D, Hd, C);
        const FrmapHeadFitWork l2 = frmap_head_fit_work(wk.layer2, B, C);
        for (int i = 0; i < B; ++i)
          for (int j = 0; j < Hd; ++j) {
            const size_t at = (size_t)i * Hd + j;
            if (wk.row_src1[i] < 0) CHECK(wk.lab[i] == -1 && wk.h[at] == 0.0f && wk.da[at] == 0.0f, "a declined row %d is not empty", i);
            if (!(wk.h[at] > 0.0f) || !p.keep2.p[at] || l2.row_src[i] < 0) CHECK(wk.da[at] == 0.0f, "da (%d, %d) behind a closed gate", i, j);
          }
        if (B >= 4) CHECK(wk.row_src1[1] == -1 && wk.row_src1[2] == -1 && wk.row_src1[3] == -1 && wk.row_src1[0] >= 0, "the three bad rows");
      }
      {   // every row declined: nothing but the workspace changes, t stays
        const Problem dead(B, D, Hd, C, true);
        const Run r = steps(dead, variation, 1, 0xFF);
        CHECK(r.w1.same(dead.w1) && r.b1.same(dead.b1) && r.w2.same(dead.w2) && r.b2.same(dead.b2), "an all-declined batch moved a weight");
        for (size_t i = 0; i < r.state.n; ++i) CHECK(r.state.p[i] == 0, "an all-declined batch wrote state byte %zu", i);
      }
      ++cases;
    }
  {   // refusals: nothing is written
    const Problem p(4, 3, 5, 2, false);
    Run r = {p.w1, p.b1, p.w2, p.b2, Block<uint8_t>(frmap_head_fit_hidden_state_size(3, 5, 2, 0)), Block<uint8_t>(frmap_head_fit_hidden_workspace_size(4, 5, 2))};
    const FrmapHeadFitHyper hy = {1e-2f, 0.9f, 0.999f, 1e-8f, 0.0f, 0.0f};
#define REFUSED(word, N_, B_, D_, Hd_, C_, flags_, w1_)                                                                                          \
  do {                                                                                                                                          \
    const char* why = frmap_head_fit_hidden_step_twin(p.x.p, p.labels.p, p.rows.p, nullptr, 1.0f, nullptr, 1.0f, w1_, r.b1.p, r.w2.p, r.b2.p,    \
                                                      r.state.p, r.work.p, N_, B_, D_, Hd_, C_, hy, flags_, 0);                                 \
    CHECK(why && strstr(why, word), "accepted, or %s is not named: %s", word, why ? why : "(accepted)");                                        \
  } while (0)
    REFUSED("N", 0, 4, 3, 5, 2, 0, r.w1.p);
    REFUSED("B", p.N, 0, 3, 5, 2, 0, r.w1.p);
    REFUSED("D", p.N, 4, 65537, 5, 2, 0, r.w1.p);
    REFUSED("Hd", p.N, 4, 3, 0, 2, 0, r.w1.p);
    REFUSED("C", p.N, 4, 3, 5, FRMAP_HEAD_FIT_MAX_C + 1, 0, r.w1.p);
    REFUSED("flags", p.N, 4, 3, 5, 2, 8, r.w1.p);
    REFUSED("null pointer", p.N, 4, 3, 5, 2, 0, (float*)nullptr);
    CHECK(r.w1.same(p.w1) && r.w2.same(p.w2), "a refused call wrote the weights");
    for (size_t i = 0; i < r.state.n; ++i) CHECK(r.state.p[i] == 0, "a refused call wrote the state");
    for (size_t i = 0; i < r.work.n; ++i) CHECK(r.work.p[i] == 0, "a refused call wrote the workspace");
  }
  CHECK(frmap_head_fit_hidden_state_size(128, 512, 18, 0) == frmap_head_fit_state_size(128, 512, 0) + frmap_head_fit_state_size(512, 18, 0) &&
            frmap_head_fit_hidden_workspace_size(32, 512, 18) == 4 * (2 * 32 * 512 + 2 * 32) + frmap_head_fit_workspace_size(32, 18),
        "sizes");
  printf("%ld cases\nself check passed\n", cases);
  return 0;
}
