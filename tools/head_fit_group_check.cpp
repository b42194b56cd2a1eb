// The grouped head-fitting step's host twin (csrc/head_fit_twin.h + head_fit_rule.h + tally_rule.h and the check programs' own
// head_fit_check_common.h, nothing else) as a stand-alone program, for a build with the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> tools/head_fit_group_check.cpp -o check && ./check
// It sweeps heads x shapes (the table of tests/fit_group_cases.py) for three steps each, masks / decoupled decay / AMSGrad taken
// from the case's index, per-head hyper-parameters all different, head h's rows ending in min(h, B - 1) entries of -1.  Every
// buffer is a heap block of exactly its size - the states H strides, the workspaces H single workspaces, rows H B, keep H B D, w
// H C D, b H C, hyper 8 H - so the sanitizer sees any access outside them.  Checked on top of that:
//   * head h of the group holds the bytes of the single twin run on head h's slices alone (weights, state, workspace);
//   * the padding bytes between a state's content and the stride keep their fill;
//   * a head whose rows are all -1 keeps weights, moments and t while its neighbours advance;
//   * flag 8 leaves w, b, moments and t as they are and adds the figures a training step on a copy adds; with flag 4 it clears
//     first; two calls accumulate;
//   * refused calls write nothing.
// Exit status 0 and "self check passed" on success.
#define CHECK_SEED 2468u
#include "head_fit_check_common.h"

struct Problem {
  int N, H, B, D, C;
  Block<float> x, w, b, hyper;
  Block<int32_t> labels, rows;
  Block<uint8_t> keep;
  Problem(int H_, int B_, int D_, int C_, int dead)
      : N(B_ + 5 + H_), H(H_), B(B_), D(D_), C(C_), x((size_t)N * D_), w((size_t)H_ * C_ * D_), b((size_t)H_ * C_), hyper((size_t)H_ * 8),
        labels(N), rows((size_t)H_ * B_), keep((size_t)H_ * B_ * D_) {
    for (size_t i = 0; i < x.n; ++i) x.p[i] = small();
    for (size_t i = 0; i < w.n; ++i) w.p[i] = small() * 0.25f;
    for (size_t i = 0; i < b.n; ++i) b.p[i] = small() * 0.25f;
    for (int i = 0; i < N; ++i) labels.p[i] = (int32_t)(rnd() % (uint32_t)C);
    for (int h = 0; h < H; ++h)
      for (int i = 0; i < B; ++i) rows.p[(size_t)h * B + i] = (int32_t)((i * 7 + 3 + 2 * h) % N);
    for (size_t i = 0; i < keep.n; ++i) keep.p[i] = rnd() % 4 ? 1 : 0;
    if (B >= 6) {
      labels.p[rows.p[1]] = C;
      x.p[(size_t)rows.p[2] * D + rnd() % (uint32_t)D] = __builtin_nanf("");
      x.p[(size_t)rows.p[3] * D + D - 1] = __builtin_inff();
      labels.p[rows.p[4]] = -1;
      for (int h = 0; h < H; ++h) rows.p[(size_t)h * B] = N;
    }
    for (int h = 0; h < H; ++h) {
      const int pad = h < B - 1 ? h : B - 1;
      for (int i = B - pad; i < B; ++i) rows.p[(size_t)h * B + i] = -1;
      if (h == dead)
        for (int i = 0; i < B; ++i) rows.p[(size_t)h * B + i] = -1;
      float* r = hyper.p + (size_t)h * 8;
      r[0] = 1e-2f * (1.0f + 0.25f * h);
      r[1] = 0.9f - 0.01f * h;
      r[2] = 0.999f - 0.001f * h;
      r[3] = 1e-8f * (1 + h);
      r[4] = 5e-3f * (h + 1);
      r[5] = 0.05f * h / (float)H;
      r[6] = 1.0f / (0.75f - 0.05f * h);
      r[7] = 0.0f;
    }
  }
};

struct Run {
  Block<float> w, b;
  Block<uint8_t> state, work;
};

static int flags_of(int index, int B, int D, int C) {
  const bool ams = (index & 4) || (B == 5 && D == 2 && C == 1);
  return (ams ? FRMAP_HEAD_FIT_AMSGRAD : 0) | ((index & 2) ? FRMAP_HEAD_FIT_DECOUPLED : 0);
}

static Run group_steps(const Problem& p, int flags, bool with_keep, int n_steps, int fill) {
  const size_t stride = frmap_head_fit_group_stride(p.D, p.C, flags & FRMAP_HEAD_FIT_AMSGRAD);
  Run r = {p.w, p.b, Block<uint8_t>((size_t)p.H * stride, fill), Block<uint8_t>((size_t)p.H * frmap_head_fit_workspace_size(p.B, p.C), fill)};
  const size_t content = (size_t)FRMAP_HEAD_FIT_HEADER * 8 + 4 * ((size_t)p.C * p.D + p.C) * ((flags & FRMAP_HEAD_FIT_AMSGRAD) ? 3 : 2);
  for (int h = 0; h < p.H; ++h) memset(r.state.p + (size_t)h * stride, 0, content);          // fresh states; the padding keeps the fill
  for (int s = 0; s < n_steps; ++s) {
    const char* why = frmap_head_fit_group_step_twin(p.x.p, p.labels.p, p.rows.p, with_keep ? p.keep.p : nullptr, p.hyper.p, r.w.p, r.b.p,
                                                     r.state.p, r.work.p, p.N, p.H, p.B, p.D, p.C, flags | (s == 0 ? FRMAP_HEAD_FIT_CLEAR : 0), 0);
    CHECK(!why, "group twin refused: %s", why);
  }
  for (int h = 0; h < p.H; ++h)
    for (size_t i = content; i < stride; ++i)
      CHECK(r.state.p[(size_t)h * stride + i] == (uint8_t)fill, "head %d: padding byte %zu of the state written", h, i);
  return r;
}

int main() {
  const int Hs[] = {1, 2, 5};
  const int shapes[][3] = {{1, 1, 1}, {5, 2, 1}, {31, 3, 2}, {32, 64, 18}, {33, 65, 33}, {65, 512, 65}};
  long cases = 0;
  int index = 0;
  for (const auto& shape : shapes)
    for (int H : Hs) {
      const int B = shape[0], D = shape[1], C = shape[2];
      const int dead = (H == 5 && B == 33) ? 2 : (H == 2 && B == 5) ? 0 : -1;
      const bool with_keep = index & 1;
      const int flags = flags_of(index, B, D, C), ams = flags & FRMAP_HEAD_FIT_AMSGRAD;
      const Problem p(H, B, D, C, dead);
      const Run one = group_steps(p, flags, with_keep, 3, 0xFF), two = group_steps(p, flags, with_keep, 3, 0x5A);
      const size_t stride = frmap_head_fit_group_stride(D, C, ams), single = frmap_head_fit_state_size(D, C, ams);
      const size_t work = frmap_head_fit_workspace_size(B, C), cd = (size_t)C * D;
      CHECK(stride % 8 == 0 && stride >= single && stride < single + 8, "stride %zu of a state of %zu bytes", stride, single);
      CHECK(one.w.same(two.w) && one.b.same(two.b) && one.work.same(two.work), "H %d B %d D %d C %d: the two fills differ", H, B, D, C);
      for (int h = 0; h < H; ++h) {                      // the single twin on the slices of head h: every buffer its own exact block
        Block<float> w(cd), b(C);
        memcpy(w.p, p.w.p + (size_t)h * cd, cd * 4);
        memcpy(b.p, p.b.p + (size_t)h * C, (size_t)C * 4);
        Block<int32_t> rows(B);
        memcpy(rows.p, p.rows.p + (size_t)h * B, (size_t)B * 4);
        Block<uint8_t> keep((size_t)B * D), st(single), wk(work, 0xFF);
        memcpy(keep.p, p.keep.p + (size_t)h * B * D, (size_t)B * D);
        float ks;
        const FrmapHeadFitHyper hy = frmap_head_fit_group_hyper(p.hyper.p, h, &ks);
        for (int s = 0; s < 3; ++s)
          CHECK(!frmap_head_fit_step_twin(p.x.p, p.labels.p, rows.p, with_keep ? keep.p : nullptr, ks, w.p, b.p, st.p, wk.p, p.N, B, D, C, hy,
                                          flags | (s == 0 ? FRMAP_HEAD_FIT_CLEAR : 0), 0),
                "single twin refused");
        const size_t content = 64 + 4 * (cd + C) * (ams ? 3 : 2);
        CHECK(memcmp(w.p, one.w.p + (size_t)h * cd, cd * 4) == 0 && memcmp(b.p, one.b.p + (size_t)h * C, (size_t)C * 4) == 0,
              "H %d B %d D %d C %d head %d: weights differ from the single twin", H, B, D, C, h);
        CHECK(memcmp(st.p, one.state.p + (size_t)h * stride, content) == 0, "H %d B %d D %d C %d head %d: state differs", H, B, D, C, h);
        CHECK(memcmp(wk.p, one.work.p + (size_t)h * work, work) == 0, "H %d B %d D %d C %d head %d: workspace differs", H, B, D, C, h);
        const uint64_t* head = (const uint64_t*)(one.state.p + (size_t)h * stride);
        if (h == dead) {
          CHECK(head[FRMAP_HEAD_FIT_T] == 0 && head[FRMAP_HEAD_FIT_N] == 0 && memcmp(w.p, p.w.p + (size_t)h * cd, cd * 4) == 0, "the dead head moved");
          for (size_t i = 64; i < content; ++i) CHECK(one.state.p[(size_t)h * stride + i] == 0, "the dead head's moment byte %zu written", i);
        } else {
          CHECK(head[FRMAP_HEAD_FIT_T] == 3 && head[FRMAP_HEAD_FIT_N] >= 1 && head[FRMAP_HEAD_FIT_ROWS] == 3 * head[FRMAP_HEAD_FIT_N],
                "H %d B %d D %d C %d head %d: header t %llu n %llu", H, B, D, C, h, (unsigned long long)head[0], (unsigned long long)head[1]);
        }
      }
      {   // flag 8 after one training step: nothing but n and the figures moves; they are what a training step on a copy adds
        const Run base = group_steps(p, flags, with_keep, 1, 0);
        Run ev = {base.w, base.b, base.state, Block<uint8_t>(base.work.n, 0xFF)};
        Run tr = {base.w, base.b, base.state, Block<uint8_t>(base.work.n, 0xFF)};
        CHECK(!frmap_head_fit_group_step_twin(p.x.p, p.labels.p, p.rows.p, nullptr, p.hyper.p, ev.w.p, ev.b.p, ev.state.p, ev.work.p, p.N, H, B, D, C,
                                              flags | FRMAP_HEAD_FIT_CLEAR | FRMAP_HEAD_FIT_EVAL, 0),
              "evaluate refused");
        CHECK(!frmap_head_fit_group_step_twin(p.x.p, p.labels.p, p.rows.p, nullptr, p.hyper.p, tr.w.p, tr.b.p, tr.state.p, tr.work.p, p.N, H, B, D, C,
                                              flags | FRMAP_HEAD_FIT_CLEAR, 0),
              "training step refused");
        CHECK(ev.w.same(base.w) && ev.b.same(base.b) && ev.work.same(tr.work), "evaluate moved the weights, or its workspace is not the step's");
        for (int h = 0; h < H; ++h) {
          const uint64_t *e = (const uint64_t*)(ev.state.p + (size_t)h * stride), *t = (const uint64_t*)(tr.state.p + (size_t)h * stride),
                         *o = (const uint64_t*)(base.state.p + (size_t)h * stride);
          CHECK(e[0] == o[0] && e[1] == t[1] && e[2] == t[2] && e[3] == t[3] && e[4] == t[4] && e[2] == e[1], "head %d: figures of evaluate", h);
          CHECK(memcmp(e + 5, o + 5, stride - 40) == 0, "head %d: evaluate wrote behind the figures", h);
        }
        Run twice = {ev.w, ev.b, ev.state, ev.work};
        CHECK(!frmap_head_fit_group_step_twin(p.x.p, p.labels.p, p.rows.p, nullptr, p.hyper.p, twice.w.p, twice.b.p, twice.state.p, twice.work.p, p.N, H,
                                              B, D, C, flags | FRMAP_HEAD_FIT_EVAL, 0),
              "second evaluate refused");
        for (int h = 0; h < H; ++h) {
          const uint64_t *e = (const uint64_t*)(ev.state.p + (size_t)h * stride), *t = (const uint64_t*)(twice.state.p + (size_t)h * stride);
          CHECK(t[2] == 2 * e[2] && t[3] == 2 * e[3] && t[4] == 2 * e[4] && t[0] == e[0], "head %d: two evaluate calls accumulate", h);
        }
      }
      ++cases;
      ++index;
    }
  {   // refusals: nothing is written
    const Problem p(2, 4, 3, 2, -1);
    Run r = {p.w, p.b, Block<uint8_t>(2 * frmap_head_fit_group_stride(3, 2, 0)), Block<uint8_t>(2 * frmap_head_fit_workspace_size(4, 2))};
#define REFUSED(word, ...)                                             \
  do {                                                                 \
    const char* why = frmap_head_fit_group_step_twin(__VA_ARGS__);     \
    CHECK(why && strstr(why, word), "accepted, or %s is not named: %s", word, why ? why : "(accepted)"); \
  } while (0)
    REFUSED("H", p.x.p, p.labels.p, p.rows.p, nullptr, p.hyper.p, r.w.p, r.b.p, r.state.p, r.work.p, p.N, 0, 4, 3, 2, 0, 0);
    REFUSED("H", p.x.p, p.labels.p, p.rows.p, nullptr, p.hyper.p, r.w.p, r.b.p, r.state.p, r.work.p, p.N, 4097, 4, 3, 2, 0, 0);
    REFUSED("flags", p.x.p, p.labels.p, p.rows.p, nullptr, p.hyper.p, r.w.p, r.b.p, r.state.p, r.work.p, p.N, 2, 4, 3, 2, 16, 0);
    REFUSED("rows", p.x.p, p.labels.p, nullptr, nullptr, p.hyper.p, r.w.p, r.b.p, r.state.p, r.work.p, p.N, 2, 4, 3, 2, 0, 0);
    REFUSED("hyper", p.x.p, p.labels.p, p.rows.p, nullptr, nullptr, r.w.p, r.b.p, r.state.p, r.work.p, p.N, 2, 4, 3, 2, 0, 0);
    REFUSED("keep", p.x.p, p.labels.p, p.rows.p, p.keep.p, p.hyper.p, r.w.p, r.b.p, r.state.p, r.work.p, p.N, 2, 4, 3, 2, 8, 0);
    REFUSED("N", p.x.p, p.labels.p, p.rows.p, nullptr, p.hyper.p, r.w.p, r.b.p, r.state.p, r.work.p, 0, 2, 4, 3, 2, 0, 0);
    REFUSED("C", p.x.p, p.labels.p, p.rows.p, nullptr, p.hyper.p, r.w.p, r.b.p, r.state.p, r.work.p, p.N, 2, 4, 3, FRMAP_HEAD_FIT_MAX_C + 1, 0, 0);
    CHECK(r.w.same(p.w) && r.b.same(p.b), "a refused call wrote the weights");
    for (size_t i = 0; i < r.state.n; ++i) CHECK(r.state.p[i] == 0, "a refused call wrote the state");
    for (size_t i = 0; i < r.work.n; ++i) CHECK(r.work.p[i] == 0, "a refused call wrote the workspace");
  }
  CHECK(frmap_head_fit_group_stride(2, 1, 1) == 104 && 64 + 12 * 3 == 100 && frmap_head_fit_group_stride(2, 1, 0) == 64 + 8 * 3 &&
            frmap_head_fit_group_stride(512, 18, 0) == frmap_head_fit_state_size(512, 18, 0),
        "strides");
  printf("%ld cases\nself check passed\n", cases);
  return 0;
}
