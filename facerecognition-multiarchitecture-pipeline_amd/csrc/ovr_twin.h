// The host twin of the count kernel of ovr_rank.hip: the rule of ovr_rule.h on host memory, positive by positive, every
// counted row against it - n^2 comparisons at most, the same predicate the kernel compiles, so the words can be compared one for
// one.  Plain C++: the library compiles it into frmap_ovr_rank_counts_host, tools/ovr_rank_check.cpp into a stand-alone program.
#pragma once
#include "ovr_rule.h"

// NULL, or why the call is refused (nothing written then).  store: [C][capacity] class-major; store_labels: [capacity];
// outputs: uint64 [n] each, every word written.
inline const char* frmap_ovr_rank_counts_twin(const float* store, const int32_t* store_labels, long long n, long long capacity, int C,
                                              uint64_t* ge_same, uint64_t* ge_other, uint64_t* eq_other) {
  if (n < 0) return "n is negative";
  if (capacity < n) return "n exceeds capacity";
  if (C < 1) return "C is below 1";
  if (n == 0) return nullptr;
  if (!store || !store_labels || !ge_same || !ge_other || !eq_other) return "null pointer";
  for (long long i = 0; i < n; ++i) {
    uint64_t a = 0, b = 0, e = 0;
    const int32_t y = store_labels[i];
    if (frmap_ovr_counted(y, C)) {
      const float* col = store + (size_t)y * (size_t)capacity;
      const float s = col[i];
      for (long long j = 0; j < n; ++j) {
        const int32_t yj = store_labels[j];
        if (!frmap_ovr_counted(yj, C)) continue;
        unsigned da, db, de;
        frmap_ovr_pair(col[j], s, yj == y, &da, &db, &de);
        a += da;
        b += db;
        e += de;
      }
    }
    ge_same[i] = a;
    ge_other[i] = b;
    eq_other[i] = e;
  }
  return nullptr;
}
