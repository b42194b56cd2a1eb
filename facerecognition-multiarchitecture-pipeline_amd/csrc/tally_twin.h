// The host twin of classify_tally.hip: the accumulation rule of tally_rule.h on host memory, row by row.  pred and rank come
// from the logits (fp32 comparisons, exact anywhere); conf and loss are INPUTS - the device's own fp32 values, or any the caller
// wants tallied - so no libm enters and the twin's state can be compared with the kernel's word for word.  Plain C++: the
// library compiles it into frmap_classify_tally_host, tools/classify_tally_check.cpp into a stand-alone program.
#pragma once
#include "tally_rule.h"

// pred / rank of one row, or -1 / -1 for a declined one; *why = 1: label out of range, 2: a non-finite logit, 0: counted
inline void frmap_tally_row_host(const float* z, int32_t y, int C, int* pred, int* rank, int* why) {
  *pred = *rank = -1;
  if (y < 0 || y >= C) { *why = 1; return; }
  for (int c = 0; c < C; ++c) {
    uint32_t u;
    __builtin_memcpy(&u, z + c, 4);
    if (!frmap_tally_finite_bits(u)) { *why = 2; return; }
  }
  *why = 0;
  const float zy = z[y];
  int p = 0, r = 0;
  for (int c = 0; c < C; ++c) {
    if (z[c] > z[p]) p = c;
    r += (z[c] > zy || (c < y && z[c] == zy)) ? 1 : 0;
  }
  *pred = p;
  *rank = r;
}

// NULL, or why the call is refused (nothing written then).  row_pred / row_rank: optional outputs.
inline const char* frmap_classify_tally_twin(const float* logits, const int32_t* labels, int B, int C, int R, int n_bins,
                                             int keep_confusion, uint64_t* state, int32_t* row_pred, int32_t* row_rank,
                                             const float* row_conf, const float* row_loss) {
  if (B < 0) return "B is negative";
  if (C < 1) return "C is below 1";
  if (R < 1 || R > FRMAP_TALLY_MAX_RANKS) return "R is outside [1, 1024]";
  if (n_bins < 1 || n_bins > FRMAP_TALLY_MAX_BINS) return "n_bins is outside [1, 1024]";
  if (keep_confusion && C > FRMAP_TALLY_MAX_CONFUSION_C) return "keep_confusion with C above 4096";
  if (B == 0) return nullptr;
  if (!logits || !labels || !state || !row_conf || !row_loss) return "null pointer";
  // a counted row's conf must lie in [0, 1] and its loss be a number >= 0: anything else has no bin and no fixed point
  for (int i = 0; i < B; ++i) {
    int pred, rank, why;
    frmap_tally_row_host(logits + (size_t)i * (size_t)C, labels[i], C, &pred, &rank, &why);
    if (why) continue;
    if (!(row_conf[i] >= 0.f && row_conf[i] <= 1.f)) return "row_conf of a counted row is outside [0, 1]";
    if (!(row_loss[i] >= 0.f)) return "row_loss of a counted row is negative or NaN";
  }
  const size_t words = frmap_tally_words(C, R, n_bins, keep_confusion);
  for (int i = 0; i < B; ++i) {
    int pred, rank, why;
    frmap_tally_row_host(logits + (size_t)i * (size_t)C, labels[i], C, &pred, &rank, &why);
    if (row_pred) row_pred[i] = pred;
    if (row_rank) row_rank[i] = rank;
    if (why) {
      state[why == 1 ? FRMAP_TALLY_IGNORED : FRMAP_TALLY_NONFINITE] += 1;
      continue;
    }
    state[FRMAP_TALLY_ROWS] += 1;
    state[FRMAP_TALLY_CORRECT] += rank == 0 ? 1 : 0;
    state[FRMAP_TALLY_LOSS_Q] += frmap_tally_loss_q(row_loss[i]);
    const int bin = frmap_tally_bin(row_conf[i], n_bins);
    const uint64_t cq = frmap_tally_conf_q(row_conf[i]);
    for (int k = 0; k < FRMAP_TALLY_ROW_ADDS; ++k) {
      size_t word;
      uint64_t amount;
      frmap_tally_row_add(k, C, R, n_bins, keep_confusion, labels[i], pred, rank, bin, cq, &word, &amount);
      if (!amount) continue;
      if (word < (size_t)FRMAP_TALLY_HEADER || word >= words) return "internal: a word outside the state";   // (never: the check program sweeps it)
      state[word] += amount;
    }
  }
  return nullptr;
}
