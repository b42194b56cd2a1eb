// The classification tally (evaluate.tally_rule is the rule in plain numpy): what one row of logits and its label add to a small
// buffer of exact integer counters, from which evaluate.metrics_from_tally derives accuracy, weighted precision / recall / F1,
// top-k, the mean loss, the per-class table, the confusion matrix and the calibration bins in float64 on the host.  The integer
// half of the rule - layout, arg-max and rank, confidence bin, fixed point - is this text, for the kernel (classify_tally.hip),
// for the host twin (tally_twin.h, frmap_classify_tally_host) and for a plain C++ compiler (tools/classify_tally_check.cpp).
// Not part of the public ABI.
//
// A row i has fp32 logits z[0 .. C) and an int32 label y.
//   declined   y < 0 or y >= C: the row adds 1 to `ignored` and nothing else, whatever its logits are.  Otherwise, if any z[c]
//              is NaN, +inf or -inf: it adds 1 to `nonfinite` and nothing else.  Row records of a declined row:
//              pred = rank = -1, conf = loss = NaN.
//   counted    pred = the first arg-max (the smallest index among the maxima);
//              rank = #{c : z[c] > z[y]} + #{c < y : z[c] == z[y]}, so rank == 0 iff pred == y.  Both are comparisons of fp32
//              values, exact on any machine.
//              conf = 1 / sum_c exp(z[c] - z[pred]) and loss = max(0, log sum_c exp(z[c] - z[pred]) + (z[pred] - z[y])), both
//              in fp32: these two are the device's own values, everything below is defined on their fp32 bits.
//   bin        np.digitize(conf, np.linspace(0, 1, n_bins)) - 1, the reference's rule with its quirk: n_bins EDGES, not
//              n_bins + 1, so only conf == 1.0 falls in the last bin.  No edge array: edge_k = 1.0 for k == n_bins - 1, else
//              (double)k * (1.0 / (double)(n_bins - 1)) (bit for bit np.linspace for n_bins 2 ... 1024; the single edge of
//              n_bins == 1 is 0), and bin = #{k : edge_k <= (double)conf} - 1.
//   adds       integers only, so a tally does not depend on the order of its rows or on how they are split into launches:
//              rows += 1, correct += (rank == 0), loss_q += llrint(min((double)loss, 65536.0) * 2^24);
//              rank_hist[min(rank, R - 1)] += 1; support[y] += 1, predicted[pred] += 1, hit[y] += (rank == 0);
//              bin_count[b] += 1, bin_correct[b] += (rank == 0), bin_conf_q[b] += llrint((double)conf * 2^32);
//              confusion[y * C + pred] += 1 where the matrix is kept.
//
// State: uint64 words, zeroed by the caller.  Words 0 .. 7 are the header - rows, ignored, nonfinite, correct, loss_q and three
// reserved words that stay zero - then rank_hist[R], support[C], predicted[C], hit[C], bin_count[NB], bin_correct[NB],
// bin_conf_q[NB] and, when kept, confusion[C * C].  loss_q overflows 64 bits after 2^24 rows at the clamp (65536 * 2^24 = 2^40
// each) and after 2^34 rows of losses below 64 (2^30 each); bin_conf_q after 2^32 rows (conf <= 1).  A kept matrix is
// refused above C = 4096: 4096^2 words are 128 MiB of state.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "track_rule.h"   // FRMAP_TRACK_HD

constexpr int FRMAP_TALLY_HEADER = 8;
constexpr int FRMAP_TALLY_ROWS = 0, FRMAP_TALLY_IGNORED = 1, FRMAP_TALLY_NONFINITE = 2, FRMAP_TALLY_CORRECT = 3, FRMAP_TALLY_LOSS_Q = 4;
constexpr int FRMAP_TALLY_MAX_RANKS = 1024, FRMAP_TALLY_MAX_BINS = 1024;
constexpr int FRMAP_TALLY_MAX_CONFUSION_C = 4096;
constexpr double FRMAP_TALLY_LOSS_CLAMP = 65536.0, FRMAP_TALLY_LOSS_SCALE = 16777216.0, FRMAP_TALLY_CONF_SCALE = 4294967296.0;

FRMAP_TRACK_HD inline bool frmap_tally_shape_ok(int C, int R, int n_bins, int keep_confusion) {
  return C >= 1 && R >= 1 && R <= FRMAP_TALLY_MAX_RANKS && n_bins >= 1 && n_bins <= FRMAP_TALLY_MAX_BINS &&
         !(keep_confusion && C > FRMAP_TALLY_MAX_CONFUSION_C);
}

// word offsets of the regions, in the order of the state
FRMAP_TRACK_HD inline size_t frmap_tally_rank_hist(int, int, int) { return (size_t)FRMAP_TALLY_HEADER; }
FRMAP_TRACK_HD inline size_t frmap_tally_support(int C, int R, int nb) { return frmap_tally_rank_hist(C, R, nb) + (size_t)R; }
FRMAP_TRACK_HD inline size_t frmap_tally_predicted(int C, int R, int nb) { return frmap_tally_support(C, R, nb) + (size_t)C; }
FRMAP_TRACK_HD inline size_t frmap_tally_hit(int C, int R, int nb) { return frmap_tally_predicted(C, R, nb) + (size_t)C; }
FRMAP_TRACK_HD inline size_t frmap_tally_bin_count(int C, int R, int nb) { return frmap_tally_hit(C, R, nb) + (size_t)C; }
FRMAP_TRACK_HD inline size_t frmap_tally_bin_correct(int C, int R, int nb) { return frmap_tally_bin_count(C, R, nb) + (size_t)nb; }
FRMAP_TRACK_HD inline size_t frmap_tally_bin_conf_q(int C, int R, int nb) { return frmap_tally_bin_correct(C, R, nb) + (size_t)nb; }
FRMAP_TRACK_HD inline size_t frmap_tally_confusion(int C, int R, int nb) { return frmap_tally_bin_conf_q(C, R, nb) + (size_t)nb; }
FRMAP_TRACK_HD inline size_t frmap_tally_words(int C, int R, int nb, int keep_confusion) {
  return frmap_tally_confusion(C, R, nb) + (keep_confusion ? (size_t)C * (size_t)C : (size_t)0);
}

// false for the bits of an infinity or a NaN
FRMAP_TRACK_HD inline bool frmap_tally_finite_bits(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }

// edge k of np.linspace(0, 1, n_bins)
FRMAP_TRACK_HD inline double frmap_tally_edge(int k, int n_bins) {
  if (n_bins == 1) return 0.0;
  return k == n_bins - 1 ? 1.0 : (double)k * (1.0 / (double)(n_bins - 1));
}

// np.digitize(conf, np.linspace(0, 1, n_bins)) - 1 for a conf in [0, 1]: the edges ascend, so the count is the serial one
FRMAP_TRACK_HD inline int frmap_tally_bin(float conf, int n_bins) {
  const double c = (double)conf;
  int n = 0;
  for (int k = 0; k < n_bins; ++k) n += frmap_tally_edge(k, n_bins) <= c ? 1 : 0;
  return n - 1;
}

FRMAP_TRACK_HD inline uint64_t frmap_tally_loss_q(float loss) {
  const double l = (double)loss;
  return (uint64_t)llrint((l < FRMAP_TALLY_LOSS_CLAMP ? l : FRMAP_TALLY_LOSS_CLAMP) * FRMAP_TALLY_LOSS_SCALE);
}
FRMAP_TRACK_HD inline uint64_t frmap_tally_conf_q(float conf) { return (uint64_t)llrint((double)conf * FRMAP_TALLY_CONF_SCALE); }

// The adds of one counted row outside the header, as (word, amount) pairs: the kernel gives one lane to each, the twin walks
// them.  k = 0 .. FRMAP_TALLY_ROW_ADDS - 1; an amount of 0 is not issued.
constexpr int FRMAP_TALLY_ROW_ADDS = 8;
FRMAP_TRACK_HD inline void frmap_tally_row_add(int k, int C, int R, int nb, int keep_confusion, int y, int pred, int rank, int bin,
                                               uint64_t conf_q, size_t* word, uint64_t* amount) {
  const uint64_t ok = rank == 0 ? 1u : 0u;
  switch (k) {
    case 0: *word = frmap_tally_rank_hist(C, R, nb) + (size_t)(rank < R - 1 ? rank : R - 1); *amount = 1; break;
    case 1: *word = frmap_tally_support(C, R, nb) + (size_t)y; *amount = 1; break;
    case 2: *word = frmap_tally_predicted(C, R, nb) + (size_t)pred; *amount = 1; break;
    case 3: *word = frmap_tally_hit(C, R, nb) + (size_t)y; *amount = ok; break;
    case 4: *word = frmap_tally_bin_count(C, R, nb) + (size_t)bin; *amount = 1; break;
    case 5: *word = frmap_tally_bin_correct(C, R, nb) + (size_t)bin; *amount = ok; break;
    case 6: *word = frmap_tally_bin_conf_q(C, R, nb) + (size_t)bin; *amount = conf_q; break;
    default:
      *word = keep_confusion ? frmap_tally_confusion(C, R, nb) + (size_t)y * (size_t)C + (size_t)pred : (size_t)0;
      *amount = keep_confusion ? 1 : 0;
      break;
  }
}
