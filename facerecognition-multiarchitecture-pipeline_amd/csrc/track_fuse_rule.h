// The arithmetic and the state layout of one track-template step (frames.fuse_tracks is the rule in plain Python), for the host
// and the device alike: a track's embeddings are pooled into a decayed sum and a weight, and the template of a track is their
// quotient.  track_fuse.hip's kernel and the host twin (track_fuse_twin.h, frmap_track_fuse_host) run this text; a plain C++
// compiler takes it too (tools/track_fuse_check.cpp).  Not part of the public ABI.
//
// Every operation is float32 and rounded once: w' = fl(fl(decay w) + 1), sum' = fl(fl(decay sum) + e), template = fl(sum' / w').
// hipcc would contract decay * s + e into one FMA on the device, which rounds once where the rule rounds twice, so the two
// functions with arithmetic that could be fused turn contraction off; the division is the correctly rounded default (the library
// is not built with fast-math).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "track_rule.h"

constexpr int FRMAP_TRACK_FUSE_MAX_DIM = 4096;

// decay * s + e in two roundings
FRMAP_TRACK_HD inline float frmap_fuse_acc(float decay, float s, float e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float t = decay * s;
  return t + e;
}

FRMAP_TRACK_HD inline float frmap_fuse_mean(float s, float w) { return s / w; }

// false for the bits of an infinity or a NaN (an integer test on the exponent field: nothing a compiler could fold away)
FRMAP_TRACK_HD inline bool frmap_fuse_finite_bits(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }

// State buffer of n_streams streams of up to max_boxes tracks of dim values (frmap_track_fuse_state_bytes; all-zero bytes =
// fresh).  Every stream has TWO banks of slots: a step reads the current bank and writes the other one, because the slot of a
// track moves whenever the detector's order changes - an in-place update would overwrite slots that other tracks still read.
//   int32   meta [n_streams][2]                    = (P = slots of the current bank, the current bank 0 / 1)   at byte 0
//   int32   ids  [n_streams][2][max_boxes]          track ids, the first P of the current bank valid          at byte align16(8 * n_streams)
//   float32 w    [n_streams][2][max_boxes]          their weights                                             right after the ids
//   float32 sum  [n_streams][2][max_boxes][pitch]   their sums, pitch = dim rounded up to 4 (16-byte rows)    right after the weights
FRMAP_TRACK_HD inline size_t frmap_fuse_pitch(int dim) { return ((size_t)dim + 3) & ~(size_t)3; }
FRMAP_TRACK_HD inline size_t frmap_fuse_ids_offset(int n_streams) { return ((size_t)8 * (size_t)n_streams + 15) & ~(size_t)15; }
FRMAP_TRACK_HD inline size_t frmap_fuse_w_offset(int n_streams, int max_boxes) {
  return frmap_fuse_ids_offset(n_streams) + (size_t)8 * (size_t)n_streams * (size_t)max_boxes;
}
FRMAP_TRACK_HD inline size_t frmap_fuse_sum_offset(int n_streams, int max_boxes) {
  return frmap_fuse_w_offset(n_streams, max_boxes) + (size_t)8 * (size_t)n_streams * (size_t)max_boxes;
}
FRMAP_TRACK_HD inline size_t frmap_fuse_bytes(int n_streams, int max_boxes, int dim) {
  return frmap_fuse_sum_offset(n_streams, max_boxes) + (size_t)8 * (size_t)n_streams * (size_t)max_boxes * frmap_fuse_pitch(dim);
}
// slot index of (stream, bank, slot) in ids / w; times the pitch in sum
FRMAP_TRACK_HD inline size_t frmap_fuse_slot(int stream, int bank, int slot, int max_boxes) {
  return ((size_t)stream * 2 + (size_t)bank) * (size_t)max_boxes + (size_t)slot;
}
