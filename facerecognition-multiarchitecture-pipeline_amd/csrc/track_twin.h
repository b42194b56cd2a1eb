// The host twin of track.hip's kernel: one tracker step over n_streams streams, HOST pointers, the arithmetic of track_rule.h
// and the kernel's order of decisions, written as the plain loop the rule describes.  frmap_track_step_host (track.hip) wraps it;
// tools/track_twin_check.cpp includes it under a plain C++ compiler with the address and undefined-behaviour sanitizers.  Not
// part of the public ABI.
#pragma once
#include <string.h>

#include <vector>

#include "track_rule.h"

// nullptr = done; otherwise the reason the call is rejected, with NOTHING written (state, ids_out and rois_out untouched)
inline const char* frmap_track_step_twin(void* state, const float* boxes, const float* probs, const int32_t* counts,
                                         const int32_t* frame_hw, int n_streams, int max_boxes, double det_thresh, double iou_thresh,
                                         int32_t* ids_out, int32_t* rois_out) {
  if (n_streams < 0) return "n_streams is negative";
  if (max_boxes < 1 || max_boxes > FRMAP_TRACK_MAX_BOXES) return "max_boxes outside [1, 256]";
  if (n_streams == 0) return nullptr;
  if (!state || !boxes || !counts || !frame_hw || !ids_out || !rois_out) return "null pointer";
  for (int s = 0; s < n_streams; ++s)
    if (counts[s] < 0 || counts[s] > max_boxes) return "a stream's count lies outside [0, max_boxes]";
  int32_t* meta = (int32_t*)state;
  float* st_boxes = (float*)((char*)state + frmap_track_boxes_offset(n_streams));
  int32_t* st_ids = (int32_t*)((char*)state + frmap_track_ids_offset(n_streams, max_boxes));
  const float thr = (float)det_thresh;
  std::vector<float> prev_box;
  std::vector<int32_t> prev_id;
  std::vector<char> matched;
  for (int s = 0; s < n_streams; ++s) {
    const size_t row = (size_t)s * (size_t)max_boxes;
    const int n = counts[s];
    int32_t* ids = ids_out + row;
    int32_t* rois = rois_out + 4 * row;
    for (int i = 0; i < max_boxes; ++i) ids[i] = -1;
    memset(rois, 0, sizeof(int32_t) * 4 * (size_t)max_boxes);
    if (n == 0) continue;                                              // tracks survive a frame without detections
    int P = meta[2 * s];
    P = P < 0 ? 0 : (P > max_boxes ? max_boxes : P);
    uint32_t next_id = (uint32_t)meta[2 * s + 1];
    prev_box.assign(st_boxes + 4 * row, st_boxes + 4 * (row + (size_t)P));   // the old state is read whole before the new one is written
    prev_id.assign(st_ids + row, st_ids + row + (size_t)P);
    matched.assign((size_t)P, 0);
    int kept = 0;
    for (int i = 0; i < n; ++i) {
      const float* box = boxes + 4 * (row + (size_t)i);
      int roi[4];
      if (!frmap_track_clip(box, probs != nullptr, probs ? probs[row + (size_t)i] : 0.f, thr, frame_hw[2 * s], frame_hw[2 * s + 1], roi)) continue;
      double best = 0.0;
      int win = -1;
      for (int j = 0; j < P; ++j) {
        if (matched[(size_t)j]) continue;
        const double iou = frmap_track_iou(box, &prev_box[4 * (size_t)j]);
        if (iou > best && iou > iou_thresh) { best = iou; win = j; }
      }
      int32_t id;
      if (win >= 0) { id = prev_id[(size_t)win]; matched[(size_t)win] = 1; }
      else id = (int32_t)(next_id++);
      ids[i] = id;
      memcpy(rois + 4 * i, roi, sizeof(roi));
      memcpy(st_boxes + 4 * (row + (size_t)kept), box, 4 * sizeof(float));
      st_ids[row + (size_t)kept] = id;
      ++kept;
    }
    meta[2 * s] = kept;
    meta[2 * s + 1] = (int32_t)next_id;
  }
  return nullptr;
}
