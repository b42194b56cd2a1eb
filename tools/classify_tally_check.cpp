// The classification tally's host twin (csrc/tally_twin.h + tally_rule.h, nothing else) as a stand-alone program, for a build
// with the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> tools/classify_tally_check.cpp -o check && ./check
// It sweeps C x R x n_bins with the confusion matrix kept and not, over rows that include labels out of range, non-finite logits,
// ties, confidences on the bin edges and at both ends, and losses at and above the clamp.  The state is a heap block of exactly
// frmap_tally_words words, so the sanitizer sees any access outside it; on top of that every (word, amount) pair the rule forms is
// asserted to lie inside the state, the tally's own sums must agree (rows = sum of every histogram = sum of the matrix), a tally
// made in three calls must equal the one made in a single call and the one of the reversed rows, and refused calls must leave
// the state untouched.  Exit status 0 and "self check passed" on success.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "tally_twin.h"

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "FAILED %s: ", #cond);      \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
      exit(1);                                    \
    }                                             \
  } while (0)

static uint32_t g_seed = 12345u;
static uint32_t rnd() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return g_seed >> 8;
}
static float unit() { return (float)(rnd() & 0xFFFF) / 65536.0f; }   // [0, 1), a multiple of 2^-16

struct Rows {
  int B, C;
  std::vector<float> z, conf, loss;
  std::vector<int32_t> y;
};

static Rows make_rows(int B, int C, int n_bins) {
  Rows r;
  r.B = B;
  r.C = C;
  r.z.resize((size_t)B * C);
  r.conf.resize(B);
  r.loss.resize(B);
  r.y.resize(B);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  for (int i = 0; i < B; ++i) {
    for (int c = 0; c < C; ++c) r.z[(size_t)i * C + c] = (float)((int)(rnd() % 13) - 6) * 0.5f;   // few values: many ties
    r.y[i] = (int32_t)(rnd() % (uint32_t)C);
    switch (i % 11) {
      case 3: r.y[i] = -1; break;
      case 5: r.y[i] = C; break;
      case 6: r.y[i] = 0x7fffffff; break;
      case 7: r.z[(size_t)i * C + (rnd() % (uint32_t)C)] = nan; break;
      case 8: r.z[(size_t)i * C + (rnd() % (uint32_t)C)] = inf; break;
      case 9: r.z[(size_t)i * C + (rnd() % (uint32_t)C)] = -inf; break;
      default: break;
    }
    if (i % 22 == 14) { r.y[i] = -5; r.z[(size_t)i * C] = nan; }      // out of range AND non-finite: ignored, not nonfinite
    switch (i % 7) {
      case 0: r.conf[i] = 1.0f; break;
      case 1: r.conf[i] = 0.0f; break;
      case 2: r.conf[i] = (float)frmap_tally_edge((int)(rnd() % (uint32_t)n_bins), n_bins); break;   // on (or rounded next to) an edge
      default: r.conf[i] = unit(); break;
    }
    switch (i % 5) {
      case 0: r.loss[i] = 0.0f; break;
      case 1: r.loss[i] = 65536.0f; break;
      case 2: r.loss[i] = 3.0e9f; break;
      default: r.loss[i] = unit() * 20.0f; break;
    }
  }
  return r;
}

static std::vector<uint64_t> tally(const Rows& r, int R, int nb, int keep, const std::vector<int>& cuts, bool reversed) {
  const size_t words = frmap_tally_words(r.C, R, nb, keep);
  uint64_t* state = (uint64_t*)calloc(words, sizeof(uint64_t));      // exactly the state: the sanitizer guards both ends
  CHECK(state, "calloc of %zu words", words);
  Rows q = r;
  if (reversed) {
    for (int i = 0; i < r.B; ++i) {
      const int j = r.B - 1 - i;
      for (int c = 0; c < r.C; ++c) q.z[(size_t)i * r.C + c] = r.z[(size_t)j * r.C + c];
      q.y[i] = r.y[j];
      q.conf[i] = r.conf[j];
      q.loss[i] = r.loss[j];
    }
  }
  std::vector<int32_t> pred(r.B), rank(r.B);
  int at = 0;
  for (size_t k = 0; k <= cuts.size(); ++k) {
    const int end = k < cuts.size() ? cuts[k] : r.B;
    const char* why = frmap_classify_tally_twin(q.z.data() + (size_t)at * r.C, q.y.data() + at, end - at, r.C, R, nb, keep, state,
                                                pred.data() + at, rank.data() + at, q.conf.data() + at, q.loss.data() + at);
    CHECK(!why, "twin refused: %s", why);
    at = end;
  }
  // every pair the rule forms for these rows lies inside the state
  for (int i = 0; i < r.B; ++i) {
    if (pred[i] < 0) {
      CHECK(rank[i] == -1, "declined row %d has rank %d", i, rank[i]);
      continue;
    }
    CHECK(pred[i] < r.C && rank[i] >= 0 && rank[i] < r.C && (rank[i] == 0) == (pred[i] == q.y[i]), "row %d: pred %d rank %d label %d", i,
          pred[i], rank[i], q.y[i]);
    const int bin = frmap_tally_bin(q.conf[i], nb);
    CHECK(bin >= 0 && bin < nb, "row %d: bin %d of %d", i, bin, nb);
    for (int k = 0; k < FRMAP_TALLY_ROW_ADDS; ++k) {
      size_t word;
      uint64_t amount;
      frmap_tally_row_add(k, r.C, R, nb, keep, q.y[i], pred[i], rank[i], bin, frmap_tally_conf_q(q.conf[i]), &word, &amount);
      CHECK(!amount || (word >= (size_t)FRMAP_TALLY_HEADER && word < words), "row %d add %d: word %zu of %zu", i, k, word, words);
    }
  }
  std::vector<uint64_t> out(state, state + words);
  free(state);
  return out;
}

static uint64_t sum(const std::vector<uint64_t>& s, size_t at, size_t n) {
  uint64_t v = 0;
  for (size_t k = 0; k < n; ++k) v += s[at + k];
  return v;
}

int main() {
  const int Cs[] = {1, 2, 63, 64, 65, 1000}, Rs[] = {1, 6, 1024}, NBs[] = {1, 2, 10, 1024};
  const int B = 259;
  long cases = 0;
  for (int C : Cs)
    for (int R : Rs)
      for (int nb : NBs)
        for (int keep = 0; keep < 2; ++keep) {
          CHECK(frmap_tally_shape_ok(C, R, nb, keep), "shape %d %d %d %d", C, R, nb, keep);
          const Rows r = make_rows(B, C, nb);
          const std::vector<uint64_t> one = tally(r, R, nb, keep, {}, false);
          const std::vector<uint64_t> three = tally(r, R, nb, keep, {1, 101}, false);
          const std::vector<uint64_t> back = tally(r, R, nb, keep, {}, true);
          CHECK(one == three, "C %d R %d nb %d keep %d: 1 + 100 + 158 rows differ from 259 at once", C, R, nb, keep);
          CHECK(one == back, "C %d R %d nb %d keep %d: the reversed rows differ", C, R, nb, keep);
          const uint64_t rows = one[FRMAP_TALLY_ROWS];
          CHECK(rows + one[FRMAP_TALLY_IGNORED] + one[FRMAP_TALLY_NONFINITE] == (uint64_t)B && rows > 0 && one[FRMAP_TALLY_IGNORED] > 0 &&
                    one[FRMAP_TALLY_NONFINITE] > 0,
                "rows %llu ignored %llu nonfinite %llu", (unsigned long long)rows, (unsigned long long)one[1], (unsigned long long)one[2]);
          CHECK(one[5] == 0 && one[6] == 0 && one[7] == 0, "reserved words written");
          CHECK(sum(one, frmap_tally_rank_hist(C, R, nb), R) == rows, "rank_hist");
          CHECK(sum(one, frmap_tally_support(C, R, nb), C) == rows, "support");
          CHECK(sum(one, frmap_tally_predicted(C, R, nb), C) == rows, "predicted");
          CHECK(sum(one, frmap_tally_hit(C, R, nb), C) == one[FRMAP_TALLY_CORRECT], "hit");
          CHECK(one[frmap_tally_rank_hist(C, R, nb)] == one[FRMAP_TALLY_CORRECT] || R == 1, "rank_hist[0] is not `correct`");
          CHECK(sum(one, frmap_tally_bin_count(C, R, nb), nb) == rows, "bin_count");
          CHECK(sum(one, frmap_tally_bin_correct(C, R, nb), nb) == one[FRMAP_TALLY_CORRECT], "bin_correct");
          if (keep) CHECK(sum(one, frmap_tally_confusion(C, R, nb), (size_t)C * C) == rows, "confusion");
          ++cases;
        }
  // the bin rule at its ends, and the fixed points
  CHECK(frmap_tally_bin(1.0f, 10) == 9 && frmap_tally_bin(0.99999994f, 10) == 8 && frmap_tally_bin(0.0f, 10) == 0 && frmap_tally_bin(0.5f, 1) == 0 &&
            frmap_tally_bin(1.0f, 2) == 1 && frmap_tally_bin(0.5f, 2) == 0 && frmap_tally_bin(1.0f, 1024) == 1023,
        "bin rule");
  CHECK(frmap_tally_loss_q(3.0e9f) == (uint64_t)65536 << 24 && frmap_tally_loss_q(1.0f) == (uint64_t)1 << 24 && frmap_tally_loss_q(0.f) == 0 &&
            frmap_tally_conf_q(1.0f) == (uint64_t)1 << 32 && frmap_tally_conf_q(0.25f) == (uint64_t)1 << 30,
        "fixed point");
  // refusals: nothing is written
  {
    std::vector<uint64_t> st(frmap_tally_words(4, 6, 10, 1), 0);
    const float z[8] = {0, 1, 2, 3, 3, 2, 1, 0}, good[2] = {0.5f, 0.5f}, badc[2] = {0.5f, 1.5f}, nanl[2] = {0.5f, __builtin_nanf("")};
    const int32_t y[2] = {1, 1};                           // row 0: pred 3, rank 2; row 1: pred 0, rank 1
    int32_t p[2], q[2];
    CHECK(frmap_classify_tally_twin(z, y, 2, 0, 6, 10, 1, st.data(), p, q, good, good), "C = 0 accepted");
    CHECK(frmap_classify_tally_twin(z, y, 2, 4, 0, 10, 1, st.data(), p, q, good, good), "R = 0 accepted");
    CHECK(frmap_classify_tally_twin(z, y, 2, 4, 1025, 10, 1, st.data(), p, q, good, good), "R = 1025 accepted");
    CHECK(frmap_classify_tally_twin(z, y, 2, 4, 6, 0, 1, st.data(), p, q, good, good), "n_bins = 0 accepted");
    CHECK(frmap_classify_tally_twin(z, y, 2, 4, 6, 1025, 1, st.data(), p, q, good, good), "n_bins = 1025 accepted");
    CHECK(frmap_classify_tally_twin(z, y, 2, 4097, 6, 10, 1, st.data(), p, q, good, good), "a 4097-class matrix accepted");
    CHECK(frmap_classify_tally_twin(z, y, -1, 4, 6, 10, 1, st.data(), p, q, good, good), "B = -1 accepted");
    CHECK(frmap_classify_tally_twin(z, y, 2, 4, 6, 10, 1, st.data(), p, q, badc, good), "conf = 1.5 accepted");
    CHECK(frmap_classify_tally_twin(z, y, 2, 4, 6, 10, 1, st.data(), p, q, good, nanl), "loss = NaN accepted");
    CHECK(frmap_classify_tally_twin(z, y, 2, 4, 6, 10, 1, nullptr, p, q, good, good), "null state accepted");
    for (uint64_t w : st) CHECK(w == 0, "a refused call wrote the state");
    CHECK(!frmap_classify_tally_twin(z, y, 0, 4, 6, 10, 1, st.data(), p, q, good, good), "B = 0 refused");
    CHECK(!frmap_classify_tally_twin(z, y, 2, 4, 6, 10, 1, st.data(), nullptr, nullptr, good, good), "a good call refused");
    CHECK(st[FRMAP_TALLY_ROWS] == 2 && st[FRMAP_TALLY_CORRECT] == 0 && st[frmap_tally_confusion(4, 6, 10) + 1 * 4 + 3] == 1 &&
              st[frmap_tally_confusion(4, 6, 10) + 1 * 4 + 0] == 1 && st[frmap_tally_rank_hist(4, 6, 10) + 2] == 1 &&
              st[frmap_tally_rank_hist(4, 6, 10) + 1] == 1,
          "the two-row case");
  }
  printf("%ld cases\nself check passed\n", cases);
  return 0;
}
