// The one-vs-rest rank counts (evaluate.ovr_rank_rule is the rule in plain numpy): the integers from which evaluate.ovr_metrics
// derives the exact one-vs-rest ROC AUC and average precision of every class in float64 on the host - no sort, no curve.  This
// text is the label rule of the score store and the pair predicate, for the kernels (ovr_rank.hip), for the host twin
// (ovr_twin.h, frmap_ovr_rank_counts_host) and for a plain C++ compiler (tools/ovr_rank_check.cpp).  Not part of the public ABI.
//
// The store keeps every score, class-major: store[c * capacity + i] = score[i][c], and one int32 label per row:
//   stored label   the label y, if 0 <= y < C and every score of the row is finite;
//                  -1 (ignored) for a label outside [0, C), whatever the scores are;
//                  -2 (nonfinite) for a NaN, +inf or -inf among the scores of a row whose label is in range.
//                  These are the tally's two kinds of declined row (tally_rule.h), so rows / ignored / nonfinite agree.
// A row with a stored label in [0, C) is COUNTED (a store written by other hands may hold a label >= C: declined like the
// negative ones).  A counted row i is a positive of exactly one class, y_i; with s_i = score[i][y_i],
// over the counted rows j < n (j == i included):
//   ge_same[i]  = #{ j : y_j == y_i and score[j][y_i] >= s_i }       (>= 1)
//   ge_other[i] = #{ j : y_j != y_i and score[j][y_i] >= s_i }
//   eq_other[i] = #{ j : y_j != y_i and score[j][y_i] == s_i }
// A declined row gets 0, 0, 0 and takes part in nobody's count.  The comparisons are IEEE fp32 comparisons of the stored values,
// as floats with denormals honoured: -0.0 equals +0.0, a denormal is not zero, a NaN (which a counted row does not hold when the
// store was written by frmap_ovr_append) compares false both ways.  Integers only: the same store gives the same words.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "tally_rule.h"   // FRMAP_TRACK_HD, frmap_tally_finite_bits

constexpr int32_t FRMAP_OVR_IGNORED = -1, FRMAP_OVR_NONFINITE = -2;

// the label the store keeps for a row: `all_finite` = no score of the row is NaN or infinite (frmap_tally_finite_bits)
FRMAP_TRACK_HD inline int32_t frmap_ovr_stored_label(int32_t y, int C, bool all_finite) {
  if (y < 0 || y >= C) return FRMAP_OVR_IGNORED;
  return all_finite ? y : FRMAP_OVR_NONFINITE;
}

// whether a stored label makes its row a counted one
FRMAP_TRACK_HD inline bool frmap_ovr_counted(int32_t stored, int C) { return stored >= 0 && stored < C; }

// What a counted row j - score v in the positive's column, same = (y_j == the positive's class) - adds to the three counts of
// a positive whose score is s: each of the three is 0 or 1.
FRMAP_TRACK_HD inline void frmap_ovr_pair(float v, float s, bool same, unsigned* ge_same, unsigned* ge_other, unsigned* eq_other) {
  const bool ge = v >= s, eq = v == s;
  *ge_same = (ge && same) ? 1u : 0u;
  *ge_other = (ge && !same) ? 1u : 0u;
  *eq_other = (eq && !same) ? 1u : 0u;
}
