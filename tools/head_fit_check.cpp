// The head-fitting step's host twin (csrc/head_fit_twin.h + head_fit_rule.h + tally_rule.h and the check programs' own
// head_fit_check_common.h, nothing else) as a stand-alone program, for a build with the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> tools/head_fit_check.cpp -o check && ./check
// It sweeps B x D x C (the grid of tests/fit_cases.py) for three steps each, the optional operands and the optimiser flags taken
// from the case's index, over batches that hold one row of each declined kind.  Every buffer is a heap block of exactly its size -
// the state frmap_head_fit_state_size bytes, the workspace frmap_head_fit_workspace_size bytes, x, labels, rows, keep, w and b
// their element counts - so the sanitizer sees any access outside them.  On top of that: a second run of the same steps must give
// the same bytes; a step through `rows` must equal the step on the gathered copy; a step re-run with given_g on its own workspace
// must give the same weights and state; a batch of declined rows only must leave weights, moments and t untouched; refused calls
// must write nothing.  Exit status 0 and "self check passed" on success.
#define CHECK_SEED 12345u
#include "head_fit_check_common.h"

struct Problem {
  int N, B, D, C;
  Block<float> x, w, b;
  Block<int32_t> labels, rows;
  Block<uint8_t> keep;
  Problem(int B_, int D_, int C_)
      : N(B_ + 5), B(B_), D(D_), C(C_), x((size_t)N * D_), w((size_t)C_ * D_), b(C_), labels(N), rows(B_), keep((size_t)B_ * D_) {
    for (size_t i = 0; i < x.n; ++i) x.p[i] = small();
    for (size_t i = 0; i < w.n; ++i) w.p[i] = small() * 0.25f;
    for (int c = 0; c < C; ++c) b.p[c] = small() * 0.25f;
    for (int i = 0; i < N; ++i) labels.p[i] = (int32_t)(rnd() % (uint32_t)C);
    for (int i = 0; i < B; ++i) rows.p[i] = (int32_t)((i * 7 + 3) % N);
    for (size_t i = 0; i < keep.n; ++i) keep.p[i] = rnd() % 4 ? 1 : 0;
    if (B >= 6) {
      labels.p[rows.p[1]] = C;
      x.p[(size_t)rows.p[2] * D + rnd() % (uint32_t)D] = __builtin_nanf("");
      x.p[(size_t)rows.p[3] * D + D - 1] = __builtin_inff();
      labels.p[rows.p[4]] = -1;
      rows.p[0] = -1;
      rows.p[5] = N;
    }
  }
};

struct Run {
  Block<float> w, b;
  Block<uint8_t> state, work;
};

static Run steps(const Problem& p, int index, int n_steps, bool with_rows, bool with_keep) {
  const int flags = ((index & 4) ? FRMAP_HEAD_FIT_AMSGRAD : 0) | ((index & 8) ? FRMAP_HEAD_FIT_DECOUPLED : 0);
  const FrmapHeadFitHyper h = {1e-2f, 0.9f, 0.999f, 1e-8f, 1e-2f, (index & 16) ? 0.05f : 0.0f};
  Run r = {p.w, p.b, Block<uint8_t>(frmap_head_fit_state_size(p.D, p.C, flags & FRMAP_HEAD_FIT_AMSGRAD)),
           Block<uint8_t>(frmap_head_fit_workspace_size(p.B, p.C))};
  for (int s = 0; s < n_steps; ++s) {
    const char* why = frmap_head_fit_step_twin(p.x.p, p.labels.p, with_rows ? p.rows.p : nullptr, with_keep ? p.keep.p : nullptr, 1.0f / 0.75f,
                                               r.w.p, r.b.p, r.state.p, r.work.p, p.N, p.B, p.D, p.C, h, flags | (s == 0 ? FRMAP_HEAD_FIT_CLEAR : 0), 0);
    CHECK(!why, "twin refused: %s", why);
  }
  return r;
}

int main() {
  const int Bs[] = {1, 31, 32, 33, 65}, Ds[] = {1, 3, 64, 65, 512}, Cs[] = {1, 2, 18, 33, 65};
  long cases = 0;
  int index = 0;
  for (int B : Bs)
    for (int D : Ds)
      for (int C : Cs) {
        CHECK(frmap_head_fit_shape_ok(D, C), "shape %d %d", D, C);
        const Problem p(B, D, C);
        const bool with_rows = index & 1, with_keep = index & 2;
        const Run one = steps(p, index, 3, with_rows, with_keep), two = steps(p, index, 3, with_rows, with_keep);
        CHECK(one.w.same(two.w) && one.b.same(two.b) && one.state.same(two.state) && one.work.same(two.work), "B %d D %d C %d: two runs differ", B, D, C);
        const uint64_t* head = (const uint64_t*)one.state.p;
        const uint64_t n = head[FRMAP_HEAD_FIT_N];
        CHECK(n >= 1 && n <= (uint64_t)B && (B < 6 || !with_rows || n <= (uint64_t)B - 6) && head[FRMAP_HEAD_FIT_T] == 3 && head[FRMAP_HEAD_FIT_ROWS] == 3 * n &&
                  head[FRMAP_HEAD_FIT_CORRECT] <= 3 * n && head[5] == 0 && head[6] == 0 && head[7] == 0,
              "B %d D %d C %d: header t %llu n %llu rows %llu", B, D, C, (unsigned long long)head[0], (unsigned long long)n, (unsigned long long)head[2]);
        if (with_rows) {                                   // the gathered copy without `rows`
          Block<float> gx((size_t)B * D);
          Block<int32_t> gl(B);
          for (int i = 0; i < B; ++i) {
            const int r = p.rows.p[i];
            const bool in = r >= 0 && r < p.N;
            for (int k = 0; k < D; ++k) gx.p[(size_t)i * D + k] = in ? p.x.p[(size_t)r * D + k] : 0.0f;
            gl.p[i] = in ? p.labels.p[r] : -1;            // (a rows entry out of range: declined either way)
          }
          const int flags = ((index & 4) ? FRMAP_HEAD_FIT_AMSGRAD : 0) | ((index & 8) ? FRMAP_HEAD_FIT_DECOUPLED : 0);
          const FrmapHeadFitHyper h = {1e-2f, 0.9f, 0.999f, 1e-8f, 1e-2f, (index & 16) ? 0.05f : 0.0f};
          Run g = {p.w, p.b, Block<uint8_t>(one.state.n), Block<uint8_t>(one.work.n)};
          for (int s = 0; s < 3; ++s)
            CHECK(!frmap_head_fit_step_twin(gx.p, gl.p, nullptr, with_keep ? p.keep.p : nullptr, 1.0f / 0.75f, g.w.p, g.b.p, g.state.p, g.work.p, B, B, D,
                                            C, h, flags, 0),
                  "gathered step refused");
          CHECK(one.w.same(g.w) && one.b.same(g.b) && one.state.same(g.state), "B %d D %d C %d: rows as a view differ from the gathered copy", B, D, C);
          const FrmapHeadFitWork a = frmap_head_fit_work(one.work.p, B, C), c = frmap_head_fit_work(g.work.p, B, C);
          CHECK(memcmp(a.z, c.z, (size_t)(2 * B * C + B) * 4) == 0, "B %d D %d C %d: z, g, row_loss of the gathered copy differ", B, D, C);
        }
        {                                                  // given_g on the step's own workspace is the step
          const int flags = ((index & 4) ? FRMAP_HEAD_FIT_AMSGRAD : 0) | ((index & 8) ? FRMAP_HEAD_FIT_DECOUPLED : 0);
          const FrmapHeadFitHyper h = {1e-2f, 0.9f, 0.999f, 1e-8f, 1e-2f, (index & 16) ? 0.05f : 0.0f};
          const Run first = steps(p, index, 1, with_rows, with_keep);
          Run again = {p.w, p.b, Block<uint8_t>(first.state.n), first.work};
          CHECK(!frmap_head_fit_step_twin(p.x.p, p.labels.p, with_rows ? p.rows.p : nullptr, with_keep ? p.keep.p : nullptr, 1.0f / 0.75f, again.w.p,
                                          again.b.p, again.state.p, again.work.p, p.N, B, D, C, h, flags | FRMAP_HEAD_FIT_CLEAR, 1),
                "given_g refused");
          CHECK(first.w.same(again.w) && first.b.same(again.b) && first.state.same(again.state) && first.work.same(again.work),
                "B %d D %d C %d: given_g on the step's own workspace differs", B, D, C);
        }
        ++cases;
        ++index;
      }
  {   // only declined rows: weights, moments and t stay; the workspace is written
    Problem p(8, 5, 3);
    for (int i = 0; i < p.N; ++i) p.labels.p[i] = i % 2 ? -1 : 3;
    const Run r = steps(p, 4, 2, true, true);
    CHECK(r.w.same(p.w) && r.b.same(p.b), "all declined: the weights moved");
    for (size_t i = 0; i < r.state.n; ++i) CHECK(r.state.p[i] == 0, "all declined: state byte %zu written", i);
    const FrmapHeadFitWork k = frmap_head_fit_work(r.work.p, p.B, p.C);
    for (int i = 0; i < p.B; ++i) CHECK(k.row_src[i] == -1 && k.row_loss[i] != k.row_loss[i], "all declined: row %d", i);
  }
  {   // refusals: nothing is written
    Problem p(4, 3, 2);
    Run r = {p.w, p.b, Block<uint8_t>(frmap_head_fit_state_size(3, 2, 0)), Block<uint8_t>(frmap_head_fit_workspace_size(4, 2))};
    const FrmapHeadFitHyper h = {1e-2f, 0.9f, 0.999f, 1e-8f, 0.f, 0.f};
#define REFUSED(...) CHECK(frmap_head_fit_step_twin(__VA_ARGS__), "accepted")
    REFUSED(p.x.p, p.labels.p, nullptr, nullptr, 1.f, r.w.p, r.b.p, r.state.p, r.work.p, 0, 4, 3, 2, h, 0, 0);
    REFUSED(p.x.p, p.labels.p, nullptr, nullptr, 1.f, r.w.p, r.b.p, r.state.p, r.work.p, 9, 0, 3, 2, h, 0, 0);
    REFUSED(p.x.p, p.labels.p, nullptr, nullptr, 1.f, r.w.p, r.b.p, r.state.p, r.work.p, 9, 4, 0, 2, h, 0, 0);
    REFUSED(p.x.p, p.labels.p, nullptr, nullptr, 1.f, r.w.p, r.b.p, r.state.p, r.work.p, 9, 4, 3, 0, h, 0, 0);
    REFUSED(p.x.p, p.labels.p, nullptr, nullptr, 1.f, r.w.p, r.b.p, r.state.p, r.work.p, 9, 4, 3, FRMAP_HEAD_FIT_MAX_C + 1, h, 0, 0);
    REFUSED(p.x.p, p.labels.p, nullptr, nullptr, 1.f, r.w.p, r.b.p, r.state.p, r.work.p, 9, 4, 3, 2, h, 8, 0);
    REFUSED(p.x.p, p.labels.p, nullptr, nullptr, 1.f, r.w.p, r.b.p, nullptr, r.work.p, 9, 4, 3, 2, h, 0, 0);
    REFUSED(nullptr, p.labels.p, nullptr, nullptr, 1.f, r.w.p, r.b.p, r.state.p, r.work.p, 9, 4, 3, 2, h, 0, 0);
    CHECK(r.w.same(p.w) && r.b.same(p.b), "a refused call wrote the weights");
    for (size_t i = 0; i < r.state.n; ++i) CHECK(r.state.p[i] == 0, "a refused call wrote the state");
    for (size_t i = 0; i < r.work.n; ++i) CHECK(r.work.p[i] == 0, "a refused call wrote the workspace");
  }
  // the sizes, the scalars and the update on values worked by hand
  CHECK(frmap_head_fit_state_size(512, 18, 0) == 64 + 4 * 2 * (512 * 18 + 18) && frmap_head_fit_state_size(3, 1, 1) == 64 + 4 * 3 * 4 &&
            frmap_head_fit_state_size(1, 1, 0) == 80 && frmap_head_fit_workspace_size(32, 18) == 4 * (2 * 32 * 18 + 64),
        "sizes");
  CHECK(frmap_head_fit_powi(0.5, 10) == 1.0 / 1024 && frmap_head_fit_powi(0.9, 0) == 1.0 && frmap_head_fit_powi(3.0, 5) == 243.0, "powi");
  {
    const FrmapHeadFitHyper h = {0.5f, 0.5f, 0.75f, 0.0f, 0.0f, 0.0f};
    const FrmapHeadFitAdam a = frmap_head_fit_adam_scalars(1, h, 0);         // bc1 = 0.5, bc2 = 0.25: step 1, sqrt 0.5
    float p = 1.0f, m = 0.0f, v = 0.0f;
    frmap_head_fit_adam(a, 2.0f, &p, &m, &v, nullptr);                      // m = 1, v = 1, denom = 1 / 0.5 = 2, p = 1 - 1 * 0.5
    CHECK(a.step_size == 1.0f && a.bc2_sqrt == 0.5f && m == 1.0f && v == 1.0f && p == 0.5f, "adam by hand: step %g sqrt %g m %g v %g p %g", a.step_size,
          a.bc2_sqrt, m, v, p);
  }
  printf("%ld cases\nself check passed\n", cases);
  return 0;
}
