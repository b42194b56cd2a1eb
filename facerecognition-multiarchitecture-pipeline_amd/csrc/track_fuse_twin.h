// The host twin of track_fuse.hip's kernel: one track-template step over n_streams streams, HOST pointers, the arithmetic and the
// layout of track_fuse_rule.h, written as the plain loop the rule describes.  frmap_track_fuse_host (track_fuse.hip) wraps it;
// tools/track_fuse_check.cpp includes it under a plain C++ compiler with the address and undefined-behaviour sanitizers.  Not
// part of the public ABI.
#pragma once
#include <string.h>

#include <vector>

#include "track_fuse_rule.h"

// nullptr = done; otherwise the reason the call is rejected, with NOTHING written (state, fused and frames_out untouched)
inline const char* frmap_track_fuse_twin(void* state, const int32_t* ids, const int32_t* counts, const float* emb, const int32_t* rows,
                                         int n_rows, int n_streams, int max_boxes, int dim, float decay, float* fused,
                                         float* frames_out) {
  if (n_streams < 0) return "n_streams is negative";
  if (max_boxes < 1 || max_boxes > FRMAP_TRACK_MAX_BOXES) return "max_boxes outside [1, 256]";
  if (dim < 1 || dim > FRMAP_TRACK_FUSE_MAX_DIM) return "dim outside [1, 4096]";
  if (n_rows < 0) return "n_rows is negative";
  if (!(decay > 0.f && decay <= 1.f)) return "decay outside (0, 1]";
  if (n_streams == 0) return n_rows ? "rows without streams" : nullptr;
  if (!state || !ids || !counts) return "null pointer";
  if (n_rows && (!emb || !rows || !fused || !frames_out)) return "null pointer";
  for (int s = 0; s < n_streams; ++s)
    if (counts[s] < 0 || counts[s] > max_boxes) return "a stream's count lies outside [0, max_boxes]";
  const size_t M = (size_t)max_boxes, D = (size_t)dim;
  std::vector<int32_t> row_of((size_t)n_streams * M, -1);                // (stream, detection) -> its row
  for (int r = 0; r < n_rows; ++r) {
    const int32_t s = rows[2 * (size_t)r], i = rows[2 * (size_t)r + 1];
    if (s < 0 || s >= n_streams) return "a row names a stream outside [0, n_streams)";
    if (i < 0 || i >= counts[s]) return "a row names a detection outside [0, counts[stream])";
    if (row_of[(size_t)s * M + (size_t)i] >= 0) return "two rows name the same detection";
    row_of[(size_t)s * M + (size_t)i] = r;
  }
  int32_t* meta = (int32_t*)state;
  int32_t* st_id = (int32_t*)((char*)state + frmap_fuse_ids_offset(n_streams));
  float* st_w = (float*)((char*)state + frmap_fuse_w_offset(n_streams, max_boxes));
  float* st_sum = (float*)((char*)state + frmap_fuse_sum_offset(n_streams, max_boxes));
  const size_t pitch = frmap_fuse_pitch(dim);
  for (int s = 0; s < n_streams; ++s) {
    const int n = counts[s];
    if (n == 0) continue;                                                // tracks survive a frame without detections
    int P = meta[2 * s];
    P = P < 0 ? 0 : (P > max_boxes ? max_boxes : P);
    const int bank = meta[2 * s + 1] & 1;
    const size_t old0 = frmap_fuse_slot(s, bank, 0, max_boxes);
    int kept = 0;
    for (int i = 0; i < n; ++i) {
      const int32_t id = ids[(size_t)s * M + (size_t)i];
      const int32_t r = row_of[(size_t)s * M + (size_t)i];
      const float* e = r >= 0 ? emb + (size_t)r * D : nullptr;
      bool pass = true;                                                  // the row (if any) goes back as it came, frames = 0
      if (id >= 0) {
        int j = -1;
        for (int q = 0; q < P && j < 0; ++q)
          if (st_id[old0 + (size_t)q] == id) j = q;
        bool finite = e != nullptr;
        for (size_t d = 0; finite && d < D; ++d) {
          uint32_t u;
          memcpy(&u, e + d, 4);
          finite = frmap_fuse_finite_bits(u);
        }
        const size_t dst = frmap_fuse_slot(s, bank ^ 1, kept, max_boxes);
        const float* so = j >= 0 ? st_sum + (old0 + (size_t)j) * pitch : nullptr;
        float* sn = st_sum + dst * pitch;
        float w2;
        if (finite) {
          w2 = j >= 0 ? frmap_fuse_acc(decay, st_w[old0 + (size_t)j], 1.f) : 1.f;
          for (size_t d = 0; d < D; ++d) sn[d] = j >= 0 ? frmap_fuse_acc(decay, so[d], e[d]) : e[d];
        } else if (j >= 0) {                                             // carried over unchanged
          w2 = st_w[old0 + (size_t)j];
          memcpy(sn, so, 4 * D);
        } else {                                                         // a new id that has nothing to pool yet
          w2 = 0.f;
          memset(sn, 0, 4 * D);
        }
        st_id[dst] = id;
        st_w[dst] = w2;
        ++kept;
        if (finite && !(w2 == 0.f)) {
          pass = false;
          for (size_t d = 0; d < D; ++d) fused[(size_t)r * D + d] = frmap_fuse_mean(sn[d], w2);
          frames_out[r] = w2;
        }
      }
      if (pass && r >= 0) {
        memcpy(fused + (size_t)r * D, e, 4 * D);
        frames_out[r] = 0.f;
      }
    }
    meta[2 * s] = kept;
    meta[2 * s + 1] = bank ^ 1;
  }
  return nullptr;
}
