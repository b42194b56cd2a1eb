// The one-vs-rest rank counts' host twin (csrc/ovr_twin.h + ovr_rule.h, nothing else of the project's) as a stand-alone
// program, for a build with the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> tools/ovr_rank_check.cpp -o check && ./check
// It sweeps N x C x three kinds of score (continuous, quantised to 1/4, all equal) over rows that include labels out of range and
// non-finite scores.  The store, the labels and the three outputs are heap blocks of exactly the sizes the call is given, so the
// sanitizer sees any access outside them; the capacity is three rows more than n, and the rows past n hold NaN and a label in
// range, which must not be read.  On top of that: a declined row has 0, 0, 0; a counted row has 1 <= ge_same <= P_c,
// eq_other <= ge_other <= N_c; an all-equal store has (P_c, N_c, N_c) everywhere; the reversed rows give the reversed integers; a
// refused call leaves the outputs untouched; the label rule is checked value by value.  Exit status 0 and "self check passed".
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ovr_twin.h"

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "FAILED %s: ", #cond);      \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
      exit(1);                                    \
    }                                             \
  } while (0)

static uint32_t g_seed = 2463534242u;
static uint32_t rnd() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return g_seed >> 8;
}

struct Rows {
  long long N;
  int C;
  std::vector<float> z;        // [N][C], row-major: what an append is given
  std::vector<int32_t> y;
};

static Rows make_rows(long long N, int C, int kind) {
  Rows r;
  r.N = N;
  r.C = C;
  r.z.resize((size_t)N * C);
  r.y.resize((size_t)N);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  for (long long i = 0; i < N; ++i) {
    for (int c = 0; c < C; ++c) {
      float v = 0.375f;
      if (kind == 0) v = (float)(rnd() & 0xFFFFF) / 1048576.0f - 0.5f;
      if (kind == 1) v = (float)(rnd() % 5) * 0.25f;
      r.z[(size_t)i * C + c] = v;
    }
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
    if (i % 22 == 14) { r.y[i] = -5; r.z[(size_t)i * C] = nan; }
  }
  return r;
}

struct Counts {
  std::vector<uint64_t> a, b, e;
  std::vector<int32_t> stored;
};

static Counts count(const Rows& r, bool reversed) {
  const long long N = r.N, cap = N + 3;
  const int C = r.C;
  float* store = (float*)malloc((size_t)C * cap * sizeof(float));          // exactly the store: the sanitizer guards both ends
  int32_t* stored = (int32_t*)malloc((size_t)cap * sizeof(int32_t));
  uint64_t* out[3];
  for (auto& o : out) o = (uint64_t*)malloc((size_t)(N ? N : 1) * sizeof(uint64_t));
  CHECK(store && stored && out[0] && out[1] && out[2], "malloc");
  for (long long i = 0; i < cap; ++i) {
    const long long src = reversed ? N - 1 - i : i;
    bool fin = true;
    for (int c = 0; c < C; ++c) {
      const float v = i < N ? r.z[(size_t)src * C + c] : __builtin_nanf("");
      uint32_t u;
      __builtin_memcpy(&u, &v, 4);
      fin = fin && frmap_tally_finite_bits(u);
      store[(size_t)c * cap + i] = v;
    }
    stored[i] = i < N ? frmap_ovr_stored_label(r.y[src], C, fin) : 0;        // past n: a label in range over NaN scores - never read
  }
  for (auto& o : out)
    for (long long i = 0; i < N; ++i) o[i] = 0xA5A5A5A5A5A5A5A5ull;           // the call writes every word itself
  const char* why = frmap_ovr_rank_counts_twin(store, stored, N, cap, C, out[0], out[1], out[2]);
  CHECK(!why, "twin refused: %s", why);
  Counts k;
  k.a.assign(out[0], out[0] + N);
  k.b.assign(out[1], out[1] + N);
  k.e.assign(out[2], out[2] + N);
  k.stored.assign(stored, stored + N);
  free(store);
  free(stored);
  for (auto& o : out) free(o);
  return k;
}

int main() {
  const long long Ns[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 1025};
  const int Cs[] = {1, 2, 3, 36, 65};
  long cases = 0;
  for (long long N : Ns)
    for (int C : Cs)
      for (int kind = 0; kind < 3; ++kind) {
        const Rows r = make_rows(N, C, kind);
        const Counts k = count(r, false), back = count(r, true);
        std::vector<uint64_t> support((size_t)C, 0);
        uint64_t rows = 0, ignored = 0, nonfinite = 0;
        for (long long i = 0; i < N; ++i) {
          if (k.stored[i] >= 0) { ++support[(size_t)k.stored[i]]; ++rows; }
          ignored += k.stored[i] == FRMAP_OVR_IGNORED ? 1 : 0;
          nonfinite += k.stored[i] == FRMAP_OVR_NONFINITE ? 1 : 0;
          CHECK(k.stored[i] >= FRMAP_OVR_NONFINITE && k.stored[i] < C, "row %lld: stored label %d", i, k.stored[i]);
        }
        CHECK(rows + ignored + nonfinite == (uint64_t)N, "rows %llu ignored %llu nonfinite %llu of %lld", (unsigned long long)rows,
              (unsigned long long)ignored, (unsigned long long)nonfinite, N);
        if (N >= 64) CHECK(rows > 0 && ignored > 0 && nonfinite > 0, "N %lld C %d: a kind of row is missing", N, C);
        for (long long i = 0; i < N; ++i) {
          const uint64_t a = k.a[i], b = k.b[i], e = k.e[i];
          CHECK(a == back.a[N - 1 - i] && b == back.b[N - 1 - i] && e == back.e[N - 1 - i], "N %lld C %d kind %d row %lld: the reversed rows differ",
                N, C, kind, i);
          if (k.stored[i] < 0) {
            CHECK(a == 0 && b == 0 && e == 0, "declined row %lld has counts", i);
            continue;
          }
          const uint64_t P = support[(size_t)k.stored[i]], Nn = rows - P;
          CHECK(a >= 1 && a <= P && b <= Nn && e <= b, "N %lld C %d kind %d row %lld: %llu %llu %llu with P %llu N %llu", N, C, kind, i,
                (unsigned long long)a, (unsigned long long)b, (unsigned long long)e, (unsigned long long)P, (unsigned long long)Nn);
          if (kind == 2) CHECK(a == P && b == Nn && e == Nn, "all-equal store, row %lld: %llu %llu %llu", i, (unsigned long long)a,
                               (unsigned long long)b, (unsigned long long)e);
        }
        ++cases;
      }
  // the pair predicate on the values that matter
  {
    unsigned a, b, e;
    const float den = 1.4e-45f, nan = __builtin_nanf("");
    frmap_ovr_pair(-0.0f, 0.0f, true, &a, &b, &e);
    CHECK(a == 1 && b == 0 && e == 0, "-0.0 >= +0.0 among the same class");
    frmap_ovr_pair(0.0f, -0.0f, false, &a, &b, &e);
    CHECK(a == 0 && b == 1 && e == 1, "+0.0 == -0.0 across classes");
    frmap_ovr_pair(den, 0.0f, false, &a, &b, &e);
    CHECK(a == 0 && b == 1 && e == 0, "a denormal is above zero, not equal to it");
    frmap_ovr_pair(0.0f, den, false, &a, &b, &e);
    CHECK(a == 0 && b == 0 && e == 0, "zero is below a denormal");
    frmap_ovr_pair(nan, 0.0f, false, &a, &b, &e);
    CHECK(a == 0 && b == 0 && e == 0, "NaN compares false");
    frmap_ovr_pair(3.4028235e38f, 3.4028235e38f, true, &a, &b, &e);
    CHECK(a == 1 && b == 0 && e == 0, "FLT_MAX against itself");
    CHECK(frmap_ovr_stored_label(-1, 3, true) == -1 && frmap_ovr_stored_label(3, 3, true) == -1 && frmap_ovr_stored_label(3, 3, false) == -1 &&
              frmap_ovr_stored_label(2, 3, false) == -2 && frmap_ovr_stored_label(2, 3, true) == 2 && frmap_ovr_stored_label(0, 1, true) == 0,
          "label rule");
    CHECK(frmap_ovr_counted(0, 1) && !frmap_ovr_counted(1, 1) && !frmap_ovr_counted(-1, 4) && !frmap_ovr_counted(-2, 4), "counted");
  }
  // refusals: nothing is written
  {
    const float store[4] = {0.5f, 0.25f, 0.5f, 0.75f};
    const int32_t lab[2] = {0, 1};
    uint64_t a[2] = {7, 7}, b[2] = {7, 7}, e[2] = {7, 7};
    CHECK(frmap_ovr_rank_counts_twin(store, lab, -1, 2, 2, a, b, e), "n = -1 accepted");
    CHECK(frmap_ovr_rank_counts_twin(store, lab, 3, 2, 2, a, b, e), "n above capacity accepted");
    CHECK(frmap_ovr_rank_counts_twin(store, lab, 2, 2, 0, a, b, e), "C = 0 accepted");
    CHECK(frmap_ovr_rank_counts_twin(nullptr, lab, 2, 2, 2, a, b, e), "null store accepted");
    CHECK(frmap_ovr_rank_counts_twin(store, lab, 2, 2, 2, a, nullptr, e), "null output accepted");
    CHECK(a[0] == 7 && a[1] == 7 && b[0] == 7 && b[1] == 7 && e[0] == 7 && e[1] == 7, "a refused call wrote an output");
    CHECK(!frmap_ovr_rank_counts_twin(nullptr, nullptr, 0, 0, 2, nullptr, nullptr, nullptr), "n = 0 refused");
    CHECK(!frmap_ovr_rank_counts_twin(store, lab, 2, 2, 2, a, b, e), "a good call refused");
    // column 0 = (0.5, 0.25), column 1 = (0.5, 0.75): row 0 (class 0) sees row 1 below it, row 1 (class 1) sees row 0 below it
    CHECK(a[0] == 1 && b[0] == 0 && e[0] == 0 && a[1] == 1 && b[1] == 0 && e[1] == 0, "the two-row case");
  }
  printf("%ld cases\nself check passed\n", cases);
  return 0;
}
